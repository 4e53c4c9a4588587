// zr_delta_host.cpp — delivering a frame as the tiles that changed since the last delivery, behind the C-ABI (zelda_render.h,
// "delivering changes"): the state (zr_ctx::delta), the host form and the device form.  A delivery is not a stage of the frame: it is two
// launches (zr_delta.hip) on the render stream behind the lighting pass of the frame enqueued last, where zr_copy_frame_async's copy
// goes, and the frame schedule knows nothing of it.
#include "zr_ctx.h"

#include <cstring>

static constexpr size_t kTileBytes = (size_t)ZR_TILE * ZR_TILE * 4;

extern "C" int zr_set_frame_delta(zr_ctx* c, int enable)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (int rc = zr_stage_idle(c, "zr_set_frame_delta", false)) return rc;
        zr_ctx::Delta& D = c->delta;
        const bool on = enable != 0;
        if (on == D.on) return ZR_OK;
        HIPCHK(c, hipSetDevice(c->device));
        if (!on) {
            HIPCHK(c, zr_sync_all(c));           // (deliveries in flight read and write what is released here)
            D.mem.release();
            D = zr_ctx::Delta();
            return ZR_OK;
        }
        if (c->cfg.tile_world > 1 || (c->cfg.flags & ZR_FLAG_PACKED_TILES))
            return zr_fail(c, ZR_ERR_UNSUPPORTED, "zr_set_frame_delta: this context's lighting pass writes packed tiles, not the frame (tile_world > 1, ZR_FLAG_PACKED_TILES)");
        const size_t n = (size_t)c->W * c->H, flag_bytes = ((size_t)c->n_tiles + 7u) / 8u * 8u;      // (k_delta_pack reads the flags eight at a time)
        ZrOwn mem;
        uint32_t *delivered = nullptr, *list = nullptr, *header = nullptr; uint8_t *packed = nullptr, *flags = nullptr;
        zr_frame_delta* h_header = nullptr;
        HIPCHK(c, mem.alloc(&delivered, n)); HIPCHK(c, mem.alloc(&packed, (size_t)c->n_tiles * kTileBytes)); HIPCHK(c, mem.alloc(&list, c->n_tiles));
        HIPCHK(c, mem.alloc(&header, 4)); HIPCHK(c, mem.alloc(&flags, flag_bytes)); HIPCHK(c, mem.host(&h_header, 1));
        HIPCHK(c, zr_fill_sync({ { delivered, 0, n * 4 }, { flags, 0, flag_bytes }, { header, 0, 16 } }));
        D.mem = std::move(mem);
        D.delivered = delivered; D.packed = packed; D.list = list; D.header = header; D.flags = flags; D.h_header = h_header;
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
    return ZR_OK;
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

// One delivery on the render stream; full and serial are the host's to know, the kernels only write them into the header
static int delta_enqueue(zr_ctx* c, uint32_t* header_dev, uint32_t* list_dev, void* packed_dev)
{
    zr_ctx::Delta& D = c->delta;
    const uint32_t serial = D.serial + 1u;
    zr_launch_frame_delta(c->d_color, D.delivered, D.flags, header_dev, list_dev, packed_dev, c->W, c->H, c->tiles_x, c->n_tiles, D.full ? 1u : 0u, serial,
                          c->stream);
    HIPCHK(c, hipGetLastError());
    D.serial = serial; D.full = false;
    return ZR_OK;
}

extern "C" int zr_read_frame_delta(zr_ctx* c, uint32_t* tiles, uint32_t cap_tiles, uint8_t* pixels, size_t bytes, zr_frame_delta* out, size_t out_bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, tiles && pixels && out && out_bytes >= sizeof(zr_frame_delta));
        ARGCHK(c, cap_tiles == c->n_tiles && bytes == (size_t)c->n_tiles * kTileBytes);
        int rc = delta_ready(c, "zr_read_frame_delta");
        if (rc == ZR_OK) rc = zr_finish(c);
        if (rc == ZR_OK) rc = delta_enqueue(c, c->delta.header, c->delta.list, c->delta.packed);
        if (rc) return rc;
        const zr_ctx::Delta& D = c->delta;
        HIPCHK(c, hipMemcpyAsync(D.h_header, D.header, sizeof(zr_frame_delta), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const zr_frame_delta h = *D.h_header;
        if (h.n_tiles > c->n_tiles) return zr_fail(c, ZR_ERR_DEVICE, "zr_read_frame_delta: more tiles listed than the frame has");
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
