// zr_overlay.hip — depth-tested line overlays in a delivered frame (zelda_render.h, "overlaying lines"; DESIGN.md section 5, "Overlaying
// lines"; zr_overlay.h has the rule).  Two launches on the render stream behind the lighting pass.
//   k_overlay_setup   a lane per segment: transform, clip, project, the major axis and the swap (zr_ov_setup) - into a 32-byte record
//                     and, beside it, the rectangle of tiles its pixels can touch as one word (rect_of_pixels); a segment that draws
//                     nothing gets the rectangle no tile lies in.
//   k_overlay_apply   a 256-thread workgroup per 32 x 32 tile, four neighbouring pixels of a row per thread (k_highlight_apply's
//                     mapping and its three alignment arms).  The workgroup scans the rectangles 256 at a time; the hits of a round
//                     are compacted IN INDEX ORDER into an LDS list - a ballot per wave, the lane's rank by the popcount of the lanes
//                     below it, the waves' bases from four LDS counters (two sets, by the round's parity: one barrier per round) - and
//                     when the next round's hits would not fit, every thread first walks the list, in order, over its own four pixels
//                     and depths (zr_ov_covers, zr_ov_depth, zr_ov_shade) and the list starts again.  So a pixel takes the segments
//                     that cross it in list order however many there are, and the result is the list's, not the schedule's.  A round
//                     without a hit costs its barrier (__syncthreads_or) and nothing else; a tile no segment reaches copies through.
// Nothing is loaded beyond x < W, y < H of the frame or the depth plane, nor beyond n records or rectangles; nothing is stored beyond
// the destination's W * H pixels or the n records.  No atomics, no scratch, global loads of the lists through ld_global (no FLAT).
// k_overlay_apply: 8 480 bytes of LDS (8 192 of the 256 records, 32 of the counters, the rest the workgroup-wide OR's), 46 VGPRs, 8 waves
// per SIMD (k_overlay_setup: 36 VGPRs, no LDS).
#include "zr_dev.h"
#include "zr_overlay.h"

static_assert(kZrOvGuard == ZR_GUARD, "the overlay clips against the rasteriser's guard band");
static_assert(kZrOvTile == 32u && TILE % kZrOvTile == 0u, "a 32 x 32 tile lies in one tile of the rectangles' grid");
constexpr uint32_t kOvList = 256u;             // records the LDS list holds: a round's hits always fit an empty list
constexpr uint32_t kOvNoRect = 0x0000FFFFu;    // tx0 = ty0 = 255, tx1 = ty1 = 0: rect_has is false for every tile

struct ZrOvCamera { float pvm[16]; float hw, hh; };

// grid: ceil(n / 256) workgroups
__global__ __launch_bounds__(256) void k_overlay_setup(const zr_overlay_segment* __restrict__ seg, uint32_t n, ZrOvCamera cam, uint32_t W, uint32_t H,
                                                       ZrOvRecord* __restrict__ recs, uint32_t* __restrict__ rects)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 s0 = ld_global((const uint4*)(seg + i)), s1 = ld_global((const uint4*)(seg + i) + 1);
    zr_overlay_segment S;
    S.a[0] = zr_u2f(s0.x); S.a[1] = zr_u2f(s0.y); S.a[2] = zr_u2f(s0.z); S.b[0] = zr_u2f(s0.w); S.b[1] = zr_u2f(s1.x); S.b[2] = zr_u2f(s1.y);
    S.rgba[0] = (uint8_t)s1.z; S.rgba[1] = (uint8_t)(s1.z >> 8); S.rgba[2] = (uint8_t)(s1.z >> 16); S.rgba[3] = (uint8_t)(s1.z >> 24);
    S.flags = s1.w;
    ZrOvRecord R;
    ZrOvBox B;
    const bool draws = zr_ov_setup(cam.pvm, cam.hw, cam.hh, W, H, S, &R, &B);
    uint4* out = (uint4*)(recs + i);
    out[0] = make_uint4((uint32_t)R.Xa, (uint32_t)R.Ya, (uint32_t)R.Xb, (uint32_t)R.Yb);
    out[1] = make_uint4(zr_f2u(R.za), zr_f2u(R.zb), R.colour, R.flags);
    rects[i] = draws ? rect_of_pixels(B.x0, B.y0, B.x1, B.y1) : kOvNoRect;
}

// the list's records [0, count) over the thread's four pixels (px .. px + 3, py), in order
__device__ __forceinline__ void overlay_walk(const ZrOvRecord* list, uint32_t count, uint4& v, const uint4& dep, int32_t px, int32_t py, float bias, uint32_t hidden)
{
    for (uint32_t j = 0u; j < count; ++j) {
        const ZrOvRecord R = list[j];
        int32_t k, dm;
        if (zr_ov_covers(R, px, py, &k, &dm)) v.x = zr_ov_shade(v.x, zr_u2f(dep.x), zr_ov_depth(R, k, dm), R.colour, R.flags, bias, hidden);
        if (zr_ov_covers(R, px + 1, py, &k, &dm)) v.y = zr_ov_shade(v.y, zr_u2f(dep.y), zr_ov_depth(R, k, dm), R.colour, R.flags, bias, hidden);
        if (zr_ov_covers(R, px + 2, py, &k, &dm)) v.z = zr_ov_shade(v.z, zr_u2f(dep.z), zr_ov_depth(R, k, dm), R.colour, R.flags, bias, hidden);
        if (zr_ov_covers(R, px + 3, py, &k, &dm)) v.w = zr_ov_shade(v.w, zr_u2f(dep.w), zr_ov_depth(R, k, dm), R.colour, R.flags, bias, hidden);
    }
}

// VEC: W % 4 == 0 (the frame's and the depth plane's loads are 16 bytes); VST: and dst is on a 16-byte boundary (so are the stores).
// grid: a workgroup per tile, row-major.
template <bool VEC, bool VST>
__global__ __launch_bounds__(256) void k_overlay_apply(const uint32_t* __restrict__ frame, const uint32_t* __restrict__ depth, const ZrOvRecord* __restrict__ recs,
                                                       const uint32_t* __restrict__ rects, uint32_t n, uint32_t* __restrict__ dst, uint32_t W, uint32_t H,
                                                       uint32_t tiles_x, float bias, uint32_t hidden)
{
    __shared__ ZrOvRecord list[kOvList];
    __shared__ uint32_t wave_hits[2][4];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t ty0 = blockIdx.x / tiles_x, x0 = (blockIdx.x - ty0 * tiles_x) * kZrOvTile, y0 = ty0 * kZrOvTile;
    const int rtx = (int)(x0 / TILE), rty = (int)(y0 / TILE);             // the tile of the rectangles' grid this one lies in
    const uint32_t px = x0 + (t & 7u) * 4u, py = y0 + (t >> 3);
    uint4 v = plane_load4<VEC>(frame, W, H, px, py);
    const uint4 dep = plane_load4<VEC>(depth, W, H, px, py);
    uint32_t count = 0u;
    for (uint32_t base = 0u, round = 0u; base < n; base += 256u, ++round) {
        const uint32_t i = base + t;
        const bool hit = i < n && rect_has(ld_global(rects + i), rtx, rty);
        const unsigned long long m = __ballot(hit);
        if (lane == 0u) wave_hits[round & 1u][wave] = (uint32_t)__popcll(m);
        if (!__syncthreads_or(hit)) continue;                             // (the same for the whole workgroup)
        const uint32_t* wh = wave_hits[round & 1u];
        const uint32_t h0 = wh[0], h1 = wh[1], h2 = wh[2], h3 = wh[3];
        const uint32_t total = h0 + h1 + h2 + h3;
        if (count + total > kOvList) {                                    // the list would overflow: the pixels consume it first
            overlay_walk(list, count, v, dep, (int32_t)px, (int32_t)py, bias, hidden);
            count = 0u;
            __syncthreads();                                              // (every thread is through with the list before it is rewritten)
        }
        if (hit) {
            const uint32_t before = wave == 0u ? 0u : wave == 1u ? h0 : wave == 2u ? h0 + h1 : h0 + h1 + h2;
            const uint32_t at = count + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            const uint4 r0 = ld_global((const uint4*)(recs + i)), r1 = ld_global((const uint4*)(recs + i) + 1);
            uint4* to = (uint4*)(list + at);
            to[0] = r0; to[1] = r1;
        }
        count += total;
    }
    if (__syncthreads_or(count != 0u)) overlay_walk(list, count, v, dep, (int32_t)px, (int32_t)py, bias, hidden);
    plane_store4<VST>(dst, W, H, px, py, v);
}

// The n segments at seg set up for the camera (pvm, hw, hh) of a W x H frame into recs and rects (n each), on st
void zr_launch_overlay_setup(const zr_overlay_segment* seg, uint32_t n, const float* pvm, float hw, float hh, uint32_t W, uint32_t H, ZrOvRecord* recs, uint32_t* rects,
                             hipStream_t st)
{
    ZrOvCamera cam;
    for (int i = 0; i < 16; ++i) cam.pvm[i] = pvm[i];
    cam.hw = hw; cam.hh = hh;
    hipLaunchKernelGGL(k_overlay_setup, dim3((n + 255u) / 256u), dim3(256), 0, st, seg, n, cam, W, H, recs, rects);
}

// `frame` (W x H, row-major RGBA8, 16-byte aligned) with the n records drawn over it against `depth` (W x H floats, 16-byte aligned) into
// dst (W x H, 4-byte aligned), on st
void zr_launch_overlay_apply(const uint32_t* frame, const float* depth, const ZrOvRecord* recs, const uint32_t* rects, uint32_t n, uint32_t* dst, uint32_t W, uint32_t H,
                             const zr_overlay_style& style, hipStream_t st)
{
    const uint32_t tiles_x = (W + kZrOvTile - 1u) / kZrOvTile, tiles_y = (H + kZrOvTile - 1u) / kZrOvTile;
    const uint32_t* dp = (const uint32_t*)depth;
    const dim3 grid(tiles_x * tiles_y), block(256);
    if (W % 4u != 0u) hipLaunchKernelGGL((k_overlay_apply<false, false>), grid, block, 0, st, frame, dp, recs, rects, n, dst, W, H, tiles_x, style.depth_bias, style.hidden_opacity);
    else if ((uintptr_t)dst % 16u != 0u) hipLaunchKernelGGL((k_overlay_apply<true, false>), grid, block, 0, st, frame, dp, recs, rects, n, dst, W, H, tiles_x, style.depth_bias, style.hidden_opacity);
    else hipLaunchKernelGGL((k_overlay_apply<true, true>), grid, block, 0, st, frame, dp, recs, rects, n, dst, W, H, tiles_x, style.depth_bias, style.hidden_opacity);
}
