// zr_delta.hip — delivering a frame as the tiles that changed since the last delivery (zelda_render.h, zr_read_frame_delta /
// zr_copy_frame_delta_async; DESIGN.md §5, "Delivering changes").  Two launches per delivery, a workgroup per 32 x 32 tile in each:
//   k_delta_mark   compares the tile of the frame with the tile of the delivered copy, writes the tile's flag byte (1: they differ, or
//                  the delivery is a full one) and brings the delivered copy up to the frame
//   k_delta_pack   a listed tile's slot is the number of flags set below its own - a count, so the list is ascending and the same from
//                  run to run by construction: no atomic decides a place - and the tile goes there, padded with 0
// Every flag is written by every delivery, with a plain store: nothing to clear, and no atomics at all.  (A bit per tile ORed into 64-bit
// words was measured first: 2 040 tiles on 32 words took k_delta_mark from 5 us to 50 us when every tile was listed.)
// Both are bandwidth-bound and nothing else: a tile is 4 KiB, a thread moves 16 bytes of it.  A frame row is W * 4 bytes, so a 16-byte
// load of it is aligned only where W % 4 == 0 (VEC); other widths load pixel by pixel.  The packed slots are 16-byte aligned always.
// Nothing is loaded or stored beyond x < W, y < H: an edge tile's threads outside the frame hold zeroes.
//
// The packed delivery (zr_read_frame_delta_packed / zr_copy_frame_delta_packed_async) sends each listed tile as a record of the tile codec
// (zr_delta_codec.h has the format) instead of its 4 096 bytes.  Three launches, k_delta_mark as it is and then
//   k_delta_measure   a listed tile's record length in 8-byte words (0: not listed; bit 15: the record is a raw one), from the widths alone
//   k_delta_encode    a listed tile's slot is the number of listed tiles below it and its offset the sum of their lengths - sums, so list,
//                     offsets and stream are the same from run to run by construction - and its record goes there
// A wave holds one row of four 8 x 8 blocks, a lane one pixel of each with its four channels in a register: a group's width is the bit
// length of the wave's OR of its values, and word k of its payload is __ballot(bit k of the lane's value) - the bit-plane transposition
// costs no LDS and no shuffles.  The tile itself is staged in LDS once (rows 40 dwords apart: a wave's 8 x 8 reads touch every bank
// once), which is where the left and upper neighbours come from.  Ordinary vector stores, no atomics, no scratch.
#include "zr_dev.h"
#include "zr_delta_codec.h"

static_assert(TILE == 32, "a thread per four pixels of a row: 8 threads per row, 32 rows, 256 threads per tile");

template <bool VEC> __global__ __launch_bounds__(256) void k_delta_mark(const uint32_t* __restrict__ frame, uint32_t* __restrict__ delivered,
                                                                        uint8_t* __restrict__ flags, uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t full)
{
    const uint32_t tile = blockIdx.x, t = threadIdx.x;
    const uint32_t px = (tile % tiles_x) * TILE + (t & 7u) * 4u, py = (tile / tiles_x) * TILE + (t >> 3);
    const uint4 f = plane_load4<VEC>(frame, W, H, px, py), d = plane_load4<VEC>(delivered, W, H, px, py);
    const bool differs = ((f.x ^ d.x) | (f.y ^ d.y) | (f.z ^ d.z) | (f.w ^ d.w)) != 0u;
    const int any = __syncthreads_or(differs ? 1 : 0);
    if (t == 0u) flags[tile] = (any || full) ? 1u : 0u;
    if (differs) plane_store4<VEC>(delivered, W, H, px, py, f);
}

// flags: one byte per tile, 0 or 1, read eight at a time (the array is padded to whole 64-bit words, the padding 0).  Tile 0's slot is 0
// whether it is listed or not, so its workgroup counts every flag instead and writes the header.
template <bool VEC> __global__ __launch_bounds__(256) void k_delta_pack(const uint32_t* __restrict__ frame, const uint8_t* __restrict__ flags,
                                                                        uint32_t* __restrict__ header, uint32_t* __restrict__ list, uint4* __restrict__ packed,
                                                                        uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t n_tiles, uint32_t full, uint32_t serial)
{
    __shared__ uint32_t part[256 / WAVE];
    const uint32_t tile = blockIdx.x, t = threadIdx.x, word = tile >> 3, byte = tile & 7u;
    const uint32_t own = flags[tile];                                   // (the same address in every lane)
    if (tile != 0u && !own) return;                                     // (the whole workgroup: nothing waits at the barrier below)
    const unsigned long long* __restrict__ fw = reinterpret_cast<const unsigned long long*>(flags);
    const uint32_t n_words = tile == 0u ? (n_tiles + 7u) / 8u : word + 1u;
    uint32_t below = 0u;
    for (uint32_t w = t; w < n_words; w += 256u) {
        const unsigned long long v = fw[w];
        below += (uint32_t)__popcll(tile != 0u && w == word ? v & ((1ull << (8u * byte)) - 1ull) : v);
    }
    const uint32_t s = (uint32_t)wave_sum((int)below);
    if ((t & (WAVE - 1u)) == 0u) part[t / WAVE] = s;
    __syncthreads();
    uint32_t slot = part[0] + part[1] + part[2] + part[3];
    if (tile == 0u) {
        if (t == 0u) { header[0] = slot; header[1] = n_tiles; header[2] = full; header[3] = serial; }
        if (!own) return;
        slot = 0u;
    }
    if (t == 0u) list[slot] = tile;
    const uint32_t px = (tile % tiles_x) * TILE + (t & 7u) * 4u, py = (tile / tiles_x) * TILE + (t >> 3);
    packed[(size_t)slot * (TILE_PIX / 4) + t] = plane_load4<VEC>(frame, W, H, px, py);
}

// ------------------------------------------------------------------------------------------------ the packed delivery

#define CODEC_ROW 40u                    // dwords between two rows of the staged tile
#define CODEC_LEN_RAW 0x8000u            // lens[]: the record is a raw one (its length is kZrCodecRawBytes / 8 words)
static_assert(kZrCodecTile == TILE && WAVE == 64 && 256 / WAVE == 4, "a wave per row of four 8 x 8 blocks, a lane per pixel of a block");

template <bool VEC> __device__ __forceinline__ void codec_stage(uint32_t* __restrict__ px, const uint32_t* __restrict__ frame, uint32_t W, uint32_t H,
                                                                uint32_t tiles_x, uint32_t tile, uint32_t t)
{
    const uint32_t x = (tile % tiles_x) * TILE + (t & 7u) * 4u, y = (tile / tiles_x) * TILE + (t >> 3);
    *reinterpret_cast<uint4*>(px + (t >> 3) * CODEC_ROW + (t & 7u) * 4u) = plane_load4<VEC>(frame, W, H, x, y);
}

// A wave's share of the staged tile: block row `wave`, the lane one pixel of each of its four blocks.  z[bx]: the pixel's zigzagged
// residuals in block bx, a byte per channel.  Returns the widths of the wave's 16 groups (16 * wave + j in nibble j: the record's own
// layout of them); sum: their total.  Bytewise arithmetic on whole pixels: (p - q) mod 256 per byte, then 2r or 2 (255 - r) + 1 = ~(2r).
__device__ __forceinline__ unsigned long long codec_wave(const uint32_t* __restrict__ px, uint32_t wave, uint32_t lane, uint32_t z[4], uint32_t& sum)
{
    const uint32_t y = wave * 8u + (lane >> 3), HI = 0x80808080u;
    unsigned long long nib = 0ull;
    sum = 0u;
#pragma unroll
    for (uint32_t bx = 0; bx < 4u; ++bx) {
        const uint32_t x = bx * 8u + (lane & 7u), at = y * CODEC_ROW + x;
        const uint32_t p = px[at], q = px[x ? at - 1u : (y ? at - CODEC_ROW : at)];      // (pixel (0, 0) predicts itself: residual 0)
        const uint32_t r = ((p | HI) - (q & ~HI)) ^ ((p ^ ~q) & HI);
        z[bx] = ((r << 1) & 0xFEFEFEFEu) ^ (((r >> 7) & 0x01010101u) * 255u);
        const uint32_t any = wave_or(z[bx]);
#pragma unroll
        for (uint32_t ch = 0; ch < 4u; ++ch) {
            const uint32_t b = 32u - (uint32_t)__clz((int)((any >> (8u * ch)) & 255u));
            nib |= (unsigned long long)b << (4u * (bx * 4u + ch));
            sum += b;
        }
    }
    return nib;
}

template <bool VEC> __global__ __launch_bounds__(256) void k_delta_measure(const uint32_t* __restrict__ frame, const uint8_t* __restrict__ flags,
                                                                           uint16_t* __restrict__ lens, uint32_t W, uint32_t H, uint32_t tiles_x)
{
    __shared__ __attribute__((aligned(16))) uint32_t px[TILE * CODEC_ROW];
    __shared__ uint32_t part[256 / WAVE];
    const uint32_t tile = blockIdx.x, t = threadIdx.x;
    if (!flags[tile]) {                                                 // (the same address in every lane: the whole workgroup leaves)
        if (t == 0u) lens[tile] = 0u;
        return;
    }
    codec_stage<VEC>(px, frame, W, H, tiles_x, tile, t);
    __syncthreads();
    uint32_t z[4], sum;
    codec_wave(px, t / WAVE, t & (WAVE - 1u), z, sum);
    if ((t & (WAVE - 1u)) == 0u) part[t / WAVE] = sum;
    __syncthreads();
    if (t == 0u) {
        const uint32_t widths = part[0] + part[1] + part[2] + part[3];
        lens[tile] = (uint16_t)(widths <= kZrCodecMaxCodedWidths ? (kZrCodecHeaderBytes + kZrCodecWidthBytes) / 8u + widths : kZrCodecRawBytes / 8u | CODEC_LEN_RAW);
    }
}

// lens: a 16-bit word per tile, read eight at a time (the array is padded to whole 16-byte words, the padding 0).  Tile 0's slot and
// offset are 0 whether it is listed or not, so its workgroup sums every tile instead and writes the header and the stream's end.
// stream: 16-byte aligned; every record starts on an 8-byte boundary.
template <bool VEC> __global__ __launch_bounds__(256) void k_delta_encode(const uint32_t* __restrict__ frame, const uint16_t* __restrict__ lens,
                                                                          uint32_t* __restrict__ header, uint32_t* __restrict__ list, uint32_t* __restrict__ offsets,
                                                                          unsigned long long* __restrict__ stream, uint32_t W, uint32_t H, uint32_t tiles_x,
                                                                          uint32_t n_tiles, uint32_t full, uint32_t serial)
{
    __shared__ __attribute__((aligned(16))) uint32_t px[TILE * CODEC_ROW];
    __shared__ uint32_t part[3][256 / WAVE], wsum[256 / WAVE];
    const uint32_t tile = blockIdx.x, t = threadIdx.x, wave = t / WAVE, lane = t & (WAVE - 1u);
    const uint32_t own = lens[tile];                                    // (the same address in every lane)
    if (tile != 0u && !own) return;                                     // (the whole workgroup: nothing waits at the barriers below)
    // place: the listed tiles below this one, their lengths, and how many of them are raw
    const uint32_t limit = tile == 0u ? n_tiles : tile;
    const uint4* __restrict__ l8 = reinterpret_cast<const uint4*>(lens);
    uint32_t below = 0u, words = 0u, raw = 0u;
    for (uint32_t w = t; w * 8u < limit; w += 256u) {
        const uint4 v = l8[w];
        const uint32_t d[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) {
            const uint32_t h = w * 8u + i < limit ? (d[i >> 1] >> (16u * (i & 1u))) & 0xFFFFu : 0u;
            below += h != 0u; words += h & (CODEC_LEN_RAW - 1u); raw += h >> 15;
        }
    }
    const uint32_t s0 = (uint32_t)wave_sum((int)below), s1 = (uint32_t)wave_sum((int)words), s2 = (uint32_t)wave_sum((int)raw);
    if (lane == 0u) { part[0][wave] = s0; part[1][wave] = s1; part[2][wave] = s2; }
    __syncthreads();
    uint32_t slot = part[0][0] + part[0][1] + part[0][2] + part[0][3], at = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    if (tile == 0u) {
        if (t == 0u) {
            header[0] = slot; header[1] = n_tiles; header[2] = full; header[3] = serial;
            header[4] = at * 8u; header[5] = part[2][0] + part[2][1] + part[2][2] + part[2][3]; header[6] = 0u; header[7] = 0u;
            offsets[slot] = at * 8u;                                    // offsets[n]: the stream's length
        }
        if (!own) return;
        slot = 0u; at = 0u;
    }
    if (t == 0u) { list[slot] = tile; offsets[slot] = at * 8u; }
    // encode: the residuals again (the tile is 4 KiB out of L2: cheaper than staging records and compacting them)
    codec_stage<VEC>(px, frame, W, H, tiles_x, tile, t);
    __syncthreads();
    uint32_t z[4], sum;
    const unsigned long long nib = codec_wave(px, wave, lane, z, sum);
    if (lane == 0u) wsum[wave] = sum;
    __syncthreads();
    unsigned long long* __restrict__ rec = stream + at;
    const uint32_t widths = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (widths > kZrCodecMaxCodedWidths) {                              // raw: the header word, then the thread's 16 bytes of the tile
        const uint4 v = *reinterpret_cast<const uint4*>(px + (t >> 3) * CODEC_ROW + (t & 7u) * 4u);
        if (t == 0u) rec[0] = (unsigned long long)px[0] | (unsigned long long)(kZrCodecRawBytes / 8u) << 32 | (unsigned long long)ZR_CODEC_RAW << 48;
        rec[1u + 2u * t] = (unsigned long long)v.x | (unsigned long long)v.y << 32;
        rec[2u + 2u * t] = (unsigned long long)v.z | (unsigned long long)v.w << 32;
        return;
    }
    const uint32_t head = (kZrCodecHeaderBytes + kZrCodecWidthBytes) / 8u;
    if (t == 0u) rec[0] = (unsigned long long)px[0] | (unsigned long long)(head + widths) << 32 | (unsigned long long)ZR_CODEC_CODED << 48;
    if (lane == 0u) rec[1u + wave] = nib;
    uint32_t word = head;                                               // the wave's first payload word: behind the waves above it
    for (uint32_t w = 0; w < wave; ++w) word += wsum[w];
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t b = (uint32_t)(nib >> (4u * j)) & 15u;           // (the same in every lane)
        if (!b) continue;
        const uint32_t v = (z[j >> 2] >> (8u * (j & 3u))) & 255u;
        unsigned long long mine = 0ull;
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            if (k >= b) break;                                          // (the whole wave: only the planes that are stored)
            const unsigned long long plane = __ballot((v >> k) & 1u);
            if (lane == k) mine = plane;
        }
        if (lane < b) rec[word + lane] = mine;
        word += b;
    }
}

// ------------------------------------------------------------------------------------------------ launchers

// One delivery on s: frame against delivered -> header (4 words), list (first n entries), packed (first n slots of 4 KiB, 16-byte aligned)
void zr_launch_frame_delta(const uint32_t* frame, uint32_t* delivered, uint8_t* flags, uint32_t* header, uint32_t* list, void* packed,
                           uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t n_tiles, uint32_t full, uint32_t serial, hipStream_t s)
{
    if (W % 4u == 0u) {
        hipLaunchKernelGGL(k_delta_mark<true>, dim3(n_tiles), dim3(256), 0, s, frame, delivered, flags, W, H, tiles_x, full);
        hipLaunchKernelGGL(k_delta_pack<true>, dim3(n_tiles), dim3(256), 0, s, frame, flags, header, list, (uint4*)packed, W, H, tiles_x, n_tiles, full, serial);
    } else {
        hipLaunchKernelGGL(k_delta_mark<false>, dim3(n_tiles), dim3(256), 0, s, frame, delivered, flags, W, H, tiles_x, full);
        hipLaunchKernelGGL(k_delta_pack<false>, dim3(n_tiles), dim3(256), 0, s, frame, flags, header, list, (uint4*)packed, W, H, tiles_x, n_tiles, full, serial);
    }
}

// One packed delivery on s: as above, but header is 8 words (zr_frame_delta_packed), offsets n + 1 entries, and stream the records back
// to back (16-byte aligned, room for n_tiles * kZrCodecRawBytes); lens: 16 bits per tile in whole 16-byte words, the padding 0
void zr_launch_frame_delta_packed(const uint32_t* frame, uint32_t* delivered, uint8_t* flags, uint16_t* lens, uint32_t* header, uint32_t* list, uint32_t* offsets,
                                  void* stream, uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t n_tiles, uint32_t full, uint32_t serial, hipStream_t s)
{
    unsigned long long* out = (unsigned long long*)stream;
    if (W % 4u == 0u) {
        hipLaunchKernelGGL(k_delta_mark<true>, dim3(n_tiles), dim3(256), 0, s, frame, delivered, flags, W, H, tiles_x, full);
        hipLaunchKernelGGL(k_delta_measure<true>, dim3(n_tiles), dim3(256), 0, s, frame, flags, lens, W, H, tiles_x);
        hipLaunchKernelGGL(k_delta_encode<true>, dim3(n_tiles), dim3(256), 0, s, frame, lens, header, list, offsets, out, W, H, tiles_x, n_tiles, full, serial);
    } else {
        hipLaunchKernelGGL(k_delta_mark<false>, dim3(n_tiles), dim3(256), 0, s, frame, delivered, flags, W, H, tiles_x, full);
        hipLaunchKernelGGL(k_delta_measure<false>, dim3(n_tiles), dim3(256), 0, s, frame, flags, lens, W, H, tiles_x);
        hipLaunchKernelGGL(k_delta_encode<false>, dim3(n_tiles), dim3(256), 0, s, frame, lens, header, list, offsets, out, W, H, tiles_x, n_tiles, full, serial);
    }
}
