// zr_delta_codec.h — the host half of the tile codec (zelda_render.h, "delivering changes, compressed"; DESIGN.md section 5, "Delivering
// changes"): the record format's constants, which the kernels of zr_delta.hip share, and the client's side of a packed delivery - check
// it, then apply it to a copy of the frame.  Plain C++17 and nothing of HIP: tests/frame_delta_codec_check.cpp compiles this header alone
// and runs the decoder under the sanitizers, over valid, truncated and mutated streams.
//
// A record is one 32 x 32 RGBA8 tile.  Per channel every value is predicted by the one to its left, in column 0 by the one above, and
// pixel (0, 0) travels in the header; the residual (p - pred) mod 256 is zigzagged (0, 255, 1, 254, ... -> 0, 1, 2, 3, ...).  The tile is
// 16 blocks of 8 x 8 pixels, a block 4 channels: group g = block * 4 + channel holds 64 values, value i = block pixel (i & 7, i >> 3),
// and has a width b = the bit length of its largest value.  Its payload is b 64-bit words, bit i of word k = bit k of value i.
//   bytes 0..3   pixel (0, 0)            4..5  u16 length of the record in 8-byte words            6..7  u16 mode: 0 coded, 1 raw
//   coded:  8..39  64 width nibbles, group g in byte g / 2, even g low;   40..  the payloads in group order:  40 + 8 * sum(b) bytes
//   raw:    8..4103  the tile's 4 096 bytes - taken exactly when the coded record would be longer than these 4 104
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

constexpr uint32_t kZrCodecTile = 32u, kZrCodecTileBytes = kZrCodecTile * kZrCodecTile * 4u;
constexpr uint32_t kZrCodecHeaderBytes = 8u, kZrCodecWidthBytes = 32u, kZrCodecGroups = 64u;
constexpr uint32_t kZrCodecRawBytes = kZrCodecHeaderBytes + kZrCodecTileBytes;                        // 4 104: no record is longer
constexpr uint32_t kZrCodecMaxCodedWidths = (kZrCodecRawBytes - kZrCodecHeaderBytes - kZrCodecWidthBytes) / 8u;      // 508
enum : uint32_t { ZR_CODEC_CODED = 0u, ZR_CODEC_RAW = 1u };

static inline uint32_t zr_codec_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static inline uint64_t zr_codec_u64(const uint8_t* p)
{
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
    return v;
}

// One record of `bytes` bytes (what its two offsets say): true when it is one the format allows, and its length word agrees
static inline bool zr_codec_record_ok(const uint8_t* rec, size_t bytes)
{
    if (bytes < kZrCodecHeaderBytes || bytes % 8u || bytes > kZrCodecRawBytes) return false;
    if ((size_t)zr_codec_u16(rec + 4) * 8u != bytes) return false;
    const uint32_t mode = zr_codec_u16(rec + 6);
    if (mode == ZR_CODEC_RAW) return bytes == kZrCodecRawBytes;
    if (mode != ZR_CODEC_CODED || bytes < kZrCodecHeaderBytes + kZrCodecWidthBytes) return false;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < kZrCodecWidthBytes; ++k) {
        const uint32_t lo = rec[8 + k] & 15u, hi = rec[8 + k] >> 4;
        if (lo > 8u || hi > 8u) return false;
        sum += lo + hi;
    }
    return (size_t)kZrCodecHeaderBytes + kZrCodecWidthBytes + 8u * (size_t)sum == bytes;
}

// A checked record -> the tile's 4 096 bytes, row by row
static inline void zr_codec_record_decode(const uint8_t* rec, uint8_t* tile)
{
    if (zr_codec_u16(rec + 6) == ZR_CODEC_RAW) { memcpy(tile, rec + kZrCodecHeaderBytes, kZrCodecTileBytes); return; }
    // the zigzagged residuals, gathered from the bit planes
    const uint8_t* payload = rec + kZrCodecHeaderBytes + kZrCodecWidthBytes;
    for (uint32_t g = 0; g < kZrCodecGroups; ++g) {
        const uint32_t b = (rec[8 + g / 2u] >> (4u * (g & 1u))) & 15u, block = g >> 2, ch = g & 3u, x0 = (block & 3u) * 8u, y0 = (block >> 2) * 8u;
        uint64_t plane[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        for (uint32_t k = 0; k < b; ++k, payload += 8) plane[k] = zr_codec_u64(payload);
        for (uint32_t i = 0; i < 64u; ++i) {
            uint32_t z = 0;
            for (uint32_t k = 0; k < b; ++k) z |= (uint32_t)((plane[k] >> i) & 1u) << k;
            tile[((y0 + (i >> 3)) * kZrCodecTile + x0 + (i & 7u)) * 4u + ch] = (uint8_t)z;
        }
    }
    // residuals -> pixels: down column 0 from pixel (0, 0), then along every row
    for (uint32_t ch = 0; ch < 4u; ++ch) {
        for (uint32_t y = 0; y < kZrCodecTile; ++y)
            for (uint32_t x = 0; x < kZrCodecTile; ++x) {
                uint8_t* p = tile + (y * kZrCodecTile + x) * 4u + ch;
                if (x == 0u && y == 0u) { *p = rec[ch]; continue; }
                const uint32_t z = *p, r = (z & 1u) ? 255u - (z >> 1) : z >> 1;
                const uint32_t pred = x ? p[-4] : p[-(ptrdiff_t)(kZrCodecTile * 4u)];
                *p = (uint8_t)(pred + r);
            }
    }
}

// A whole delivery against a width x height frame: the list ascends and stays inside the frame's tiles, the offsets start at 0, ascend
// and end inside `bytes`, and every record is one the format allows.  Reads nothing outside tiles[0..n), offsets[0..n] and stream[0..bytes).
static inline bool zr_codec_stream_ok(const uint32_t* tiles, const uint32_t* offsets, uint32_t n, const uint8_t* stream, size_t bytes, uint32_t width, uint32_t height)
{
    if (!width || !height) return false;
    const uint64_t total = (uint64_t)((width + kZrCodecTile - 1u) / kZrCodecTile) * ((height + kZrCodecTile - 1u) / kZrCodecTile);
    if (n > total || offsets[0] != 0u) return false;
    for (uint32_t k = 0; k < n; ++k) {
        if (tiles[k] >= total || (k && tiles[k] <= tiles[k - 1u])) return false;
        if (offsets[k + 1u] <= offsets[k] || offsets[k + 1u] > bytes) return false;
        if (!zr_codec_record_ok(stream + offsets[k], offsets[k + 1u] - offsets[k])) return false;
    }
    return true;
}

// The client's side: a delivery applied to its width x height x 4 copy of the frame - only pixels inside the frame are touched.  false, and
// nothing written, when zr_codec_stream_ok refuses the delivery.
static inline bool zr_codec_apply(const uint32_t* tiles, const uint32_t* offsets, uint32_t n, const uint8_t* stream, size_t bytes, uint32_t width, uint32_t height,
                                  uint8_t* client_rgba8)
{
    if (!zr_codec_stream_ok(tiles, offsets, n, stream, bytes, width, height)) return false;
    const uint32_t tiles_x = (width + kZrCodecTile - 1u) / kZrCodecTile;
    uint8_t tile[kZrCodecTileBytes];
    for (uint32_t k = 0; k < n; ++k) {
        zr_codec_record_decode(stream + offsets[k], tile);
        const uint32_t x0 = tiles[k] % tiles_x * kZrCodecTile, y0 = tiles[k] / tiles_x * kZrCodecTile;
        const uint32_t w = width - x0 < kZrCodecTile ? width - x0 : kZrCodecTile, h = height - y0 < kZrCodecTile ? height - y0 : kZrCodecTile;
        for (uint32_t y = 0; y < h; ++y)
            memcpy(client_rgba8 + ((size_t)(y0 + y) * width + x0) * 4u, tile + (size_t)y * kZrCodecTile * 4u, (size_t)w * 4u);
    }
    return true;
}
