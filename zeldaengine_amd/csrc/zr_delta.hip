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
#include "zr_dev.h"

static_assert(TILE == 32, "a thread per four pixels of a row: 8 threads per row, 32 rows, 256 threads per tile");

// The calling thread's four pixels (px .. px + 3, py) of a plane; 0 where they lie outside it.  VEC: W % 4 == 0, so px < W puts all four
// inside and the address on a 16-byte boundary.
template <bool VEC> __device__ __forceinline__ uint4 delta_load4(const uint32_t* __restrict__ plane, uint32_t W, uint32_t H, uint32_t px, uint32_t py)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (py >= H || px >= W) return v;
    const uint32_t* p = plane + (size_t)py * W + px;
    if (VEC) return *reinterpret_cast<const uint4*>(p);
    v.x = p[0];
    if (px + 1u < W) v.y = p[1];
    if (px + 2u < W) v.z = p[2];
    if (px + 3u < W) v.w = p[3];
    return v;
}
template <bool VEC> __device__ __forceinline__ void delta_store4(uint32_t* __restrict__ plane, uint32_t W, uint32_t H, uint32_t px, uint32_t py, uint4 v)
{
    if (py >= H || px >= W) return;
    uint32_t* p = plane + (size_t)py * W + px;
    if (VEC) { *reinterpret_cast<uint4*>(p) = v; return; }
    p[0] = v.x;
    if (px + 1u < W) p[1] = v.y;
    if (px + 2u < W) p[2] = v.z;
    if (px + 3u < W) p[3] = v.w;
}

template <bool VEC> __global__ __launch_bounds__(256) void k_delta_mark(const uint32_t* __restrict__ frame, uint32_t* __restrict__ delivered,
                                                                        uint8_t* __restrict__ flags, uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t full)
{
    const uint32_t tile = blockIdx.x, t = threadIdx.x;
    const uint32_t px = (tile % tiles_x) * TILE + (t & 7u) * 4u, py = (tile / tiles_x) * TILE + (t >> 3);
    const uint4 f = delta_load4<VEC>(frame, W, H, px, py), d = delta_load4<VEC>(delivered, W, H, px, py);
    const bool differs = ((f.x ^ d.x) | (f.y ^ d.y) | (f.z ^ d.z) | (f.w ^ d.w)) != 0u;
    const int any = __syncthreads_or(differs ? 1 : 0);
    if (t == 0u) flags[tile] = (any || full) ? 1u : 0u;
    if (differs) delta_store4<VEC>(delivered, W, H, px, py, f);
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
    packed[(size_t)slot * (TILE_PIX / 4) + t] = delta_load4<VEC>(frame, W, H, px, py);
}

// ------------------------------------------------------------------------------------------------ launcher

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
