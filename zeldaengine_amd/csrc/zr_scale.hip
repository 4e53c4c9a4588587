// zr_scale.hip — the frame box-filtered by an integer factor s in linear light (zelda_render.h, "delivering a scaled frame"; DESIGN.md
// section 5, "Delivering a scaled frame"; zr_scale.h has the rule and the table).  One launch, k_frame_scale: a workgroup takes one row of
// output pixels - s frame rows - and up to 1 024 frame columns of it, in two steps.
//   columns   a thread holds four neighbouring frame columns: it loads its four pixels of each of the s rows (lanes adjacent in x read
//             adjacent addresses; 16 bytes at a time where W % 4 == 0, pixel by pixel otherwise: plane_load4), looks each colour byte up
//             in T and leaves the four columns' sums, a plane per channel, in LDS
//   blocks    a thread per output pixel adds its s column sums, turns them into the pixel (zr_scale_block: eight probes of the midpoints
//             per colour channel) and stores it - a 4-byte store: the destination may be a caller's buffer aligned to no more than that
// The arms compiled for s = 2 and s = 4 (where W % 4 == 0) skip the LDS planes and the second barrier: a thread's four columns are two
// whole blocks or one, so their sums stay in its registers and it writes the two pixels, or the one, itself.
// A workgroup's first frame column is a multiple of four (SCALE_COLS / s output pixels, rounded down to a multiple of four, each s wide),
// so the 16-byte loads stay aligned whatever s is.  Nothing is loaded beyond x < W, y < H - a pixel outside reads as 0, which adds
// nothing to any sum, and n counts only the pixels inside - and nothing is stored beyond X < Wd, Y < Hd.
// The tables live in LDS, loaded once per workgroup (lanes index them apart, so a scalar or constant read would serialise): T as 16-bit
// entries, 128 dwords - ds_read_u16 goes by the dword's bank modulo 32 within a half wave and equal dwords broadcast, so four dwords
// share a bank where 32-bit entries would put eight there; the midpoints need 17 bits and are 32-bit.  The memory traffic is the
// compulsory one, W * H * 4 bytes in and Wd * Hd * 4 out (at 1920 x 1080 the time is a launch and one pass of latency, not the traffic:
// DESIGN.md section 7).  Ordinary vector loads and stores, no atomics, no scratch.
#include "zr_dev.h"
#include "zr_scale.h"

#define SCALE_COLS 1024u                 // frame columns a workgroup sums: 256 threads, four each

__constant__ uint16_t c_scale_T[256] = { ZR_SCALE_TABLE_LITERALS };

// S: the factor at compile time (2, 4), or 0 - the factor is s_any (1 .. kZrScaleMax).  per_wg: output pixels a workgroup writes
// (per_wg * s <= SCALE_COLS and a multiple of 4); chunks: workgroups per output row.  VEC needs `frame` on a 16-byte boundary.
template <uint32_t S, bool VEC> __global__ __launch_bounds__(256) void k_frame_scale(const uint32_t* __restrict__ frame, uint32_t* __restrict__ dst, uint32_t W,
                                                                                      uint32_t H, uint32_t Wd, uint32_t s_any, uint32_t per_wg, uint32_t chunks)
{
    __shared__ uint16_t T[256];
    __shared__ uint32_t mid[256];
    constexpr uint32_t R = S ? S : kZrScaleMax;
    const uint32_t s = S ? S : s_any, t = threadIdx.x;
    const uint32_t Y = blockIdx.x / chunks, X0 = (blockIdx.x % chunks) * per_wg, y0 = Y * s, px = X0 * s + 4u * t;
    T[t] = c_scale_T[t];
    mid[t] = zr_scale_midpoint(c_scale_T, t);
    uint4 v[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r)     // (the loads of all rows are in flight together; the next workgroup's columns are not this one's to load)
        v[r] = r < s && 4u * t < per_wg * s ? plane_load4<VEC>(frame, W, H, px, y0 + r) : make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    uint32_t a[4][4] = { { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u } };      // [channel][column]
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t p[4] = { v[r].x, v[r].y, v[r].z, v[r].w };
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            a[0][i] += T[p[i] & 255u]; a[1][i] += T[(p[i] >> 8) & 255u]; a[2][i] += T[(p[i] >> 16) & 255u]; a[3][i] += p[i] >> 24;
        }
    }
    const uint32_t rows = min(s, H - y0);
    if constexpr (S != 0u) {             // 2, 4: the thread's four columns are 4 / S whole blocks - their sums never leave its registers
        static_assert(4u % (S ? S : 1u) == 0u, "a compile-time factor divides the four columns a thread holds");
        if (4u * t >= per_wg * S) return;
#pragma unroll
        for (uint32_t o = 0; o < 4u / S; ++o) {
            const uint32_t X = X0 + 4u * t / S + o;
            if (X >= Wd) break;
            uint32_t sum[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
            for (uint32_t i = 0; i < S; ++i) { sum[0] += a[0][o * S + i]; sum[1] += a[1][o * S + i]; sum[2] += a[2][o * S + i]; sum[3] += a[3][o * S + i]; }
            dst[(size_t)Y * Wd + X] = zr_scale_block(mid, sum, min(S, W - X * S) * rows);
        }
    } else {                             // any factor: the column sums go through LDS, a plane per channel, and a thread per output pixel adds its s
        __shared__ __attribute__((aligned(16))) uint32_t col[4][SCALE_COLS];
#pragma unroll
        for (uint32_t ch = 0; ch < 4u; ++ch) *reinterpret_cast<uint4*>(&col[ch][4u * t]) = make_uint4(a[ch][0], a[ch][1], a[ch][2], a[ch][3]);
        __syncthreads();
        for (uint32_t j = t; j < per_wg; j += 256u) {
            const uint32_t X = X0 + j;
            if (X >= Wd) break;
            uint32_t sum[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
            for (uint32_t i = 0; i < R; ++i)
                if (i < s) { sum[0] += col[0][j * s + i]; sum[1] += col[1][j * s + i]; sum[2] += col[2][j * s + i]; sum[3] += col[3][j * s + i]; }
            dst[(size_t)Y * Wd + X] = zr_scale_block(mid, sum, min(s, W - X * s) * rows);
        }
    }
}

// `frame` (W x H, row-major RGBA8, 16-byte aligned) filtered by s (1 .. kZrScaleMax) into dst (ceil(W / s) x ceil(H / s), 4-byte aligned), on st
void zr_launch_frame_scale(const uint32_t* frame, uint32_t* dst, uint32_t W, uint32_t H, uint32_t s, hipStream_t st)
{
    const uint32_t Wd = zr_scale_extent(W, s), Hd = zr_scale_extent(H, s), per_wg = (SCALE_COLS / s) & ~3u, chunks = (Wd + per_wg - 1u) / per_wg;
    const dim3 grid(Hd * chunks), block(256);
    if (W % 4u != 0u) hipLaunchKernelGGL((k_frame_scale<0u, false>), grid, block, 0, st, frame, dst, W, H, Wd, s, per_wg, chunks);
    else if (s == 2u) hipLaunchKernelGGL((k_frame_scale<2u, true>), grid, block, 0, st, frame, dst, W, H, Wd, s, per_wg, chunks);
    else if (s == 4u) hipLaunchKernelGGL((k_frame_scale<4u, true>), grid, block, 0, st, frame, dst, W, H, Wd, s, per_wg, chunks);
    else hipLaunchKernelGGL((k_frame_scale<0u, true>), grid, block, 0, st, frame, dst, W, H, Wd, s, per_wg, chunks);
}
