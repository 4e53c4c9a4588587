// zr_scale.h — the frame box-filtered by an integer factor in linear light (zelda_render.h, "delivering a scaled frame"; DESIGN.md
// section 5, "Delivering a scaled frame"): the table, and the ONE statement of what a block of frame pixels becomes, which the kernel
// (zr_scale.hip: k_frame_scale) and the host function (zr_frame_downscale) both call.  Plain C++ and nothing of HIP: a stand-alone
// program can include it (tests/frame_scale_check.cpp does, under the sanitizers).
//
// Everything is integer arithmetic.  T[c] = floor(65535 * L(c / 255) + 1/2), L the sRGB EOTF in float64; the 256 literals below are
// normative (no entry lies within 1.6e-3 of a rounding tie; T is strictly increasing, its least gap 19).  Output pixel (X, Y) at scale s
// covers the block X s <= x < min(W, (X + 1) s), Y s <= y < min(H, (Y + 1) s) of n pixels - fewer than s * s in the last column and row:
// edge blocks average the pixels that exist.  R, G, B each: S = the sum of T[p] over the block; the result is the number of k in 1..255
// with 2 S >= (T[k - 1] + T[k]) n - the byte whose T is nearest the block's mean, ties upward.  A: floor((2 sum + n) / (2 n)).
// With n <= 64 every intermediate is below 2^24: 2 S <= 8 388 480, (T[k - 1] + T[k]) n <= 8 351 168.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZR_SCALE_FN __host__ __device__ static inline
#else
#define ZR_SCALE_FN static inline
#endif

constexpr uint32_t kZrScaleMax = 8u;     // the largest factor: a block is at most 64 pixels

#define ZR_SCALE_TABLE_LITERALS \
        0,    20,    40,    60,    80,    99,   119,   139,   159,   179,   199,   219,   241,   264,   288,   313, \
      340,   367,   396,   427,   458,   491,   526,   562,   599,   637,   677,   718,   761,   805,   851,   898, \
      947,   997,  1048,  1101,  1156,  1212,  1270,  1330,  1391,  1453,  1517,  1583,  1651,  1720,  1790,  1863, \
     1937,  2013,  2090,  2170,  2250,  2333,  2418,  2504,  2592,  2681,  2773,  2866,  2961,  3058,  3157,  3258, \
     3360,  3464,  3570,  3678,  3788,  3900,  4014,  4129,  4247,  4366,  4488,  4611,  4736,  4864,  4993,  5124, \
     5257,  5392,  5530,  5669,  5810,  5953,  6099,  6246,  6395,  6547,  6700,  6856,  7014,  7174,  7335,  7500, \
     7666,  7834,  8004,  8177,  8352,  8528,  8708,  8889,  9072,  9258,  9445,  9635,  9828, 10022, 10219, 10417, \
    10619, 10822, 11028, 11235, 11446, 11658, 11873, 12090, 12309, 12530, 12754, 12980, 13209, 13440, 13673, 13909, \
    14146, 14387, 14629, 14874, 15122, 15371, 15623, 15878, 16135, 16394, 16656, 16920, 17187, 17456, 17727, 18001, \
    18277, 18556, 18837, 19121, 19407, 19696, 19987, 20281, 20577, 20876, 21177, 21481, 21787, 22096, 22407, 22721, \
    23038, 23357, 23678, 24002, 24329, 24658, 24990, 25325, 25662, 26001, 26344, 26688, 27036, 27386, 27739, 28094, \
    28452, 28813, 29176, 29542, 29911, 30282, 30656, 31033, 31412, 31794, 32179, 32567, 32957, 33350, 33745, 34143, \
    34544, 34948, 35355, 35764, 36176, 36591, 37008, 37429, 37852, 38278, 38706, 39138, 39572, 40009, 40449, 40891, \
    41337, 41785, 42236, 42690, 43147, 43606, 44069, 44534, 45002, 45473, 45947, 46423, 46903, 47385, 47871, 48359, \
    48850, 49344, 49841, 50341, 50844, 51349, 51858, 52369, 52884, 53401, 53921, 54445, 54971, 55500, 56032, 56567, \
    57105, 57646, 58190, 58737, 59287, 59840, 60396, 60955, 61517, 62082, 62650, 63221, 63795, 64372, 64952, 65535

// The host's copy of T (the kernel keeps its own, of the same literals, where its lanes can index it)
static const uint16_t kZrScaleT[256] = { ZR_SCALE_TABLE_LITERALS };

ZR_SCALE_FN uint32_t zr_scale_extent(uint32_t extent, uint32_t s) { return (extent + s - 1u) / s; }

// mid[k] = T[k - 1] + T[k], k = 1 .. 255: twice the point between two neighbouring levels (mid[0] = 0 is never looked at)
ZR_SCALE_FN uint32_t zr_scale_midpoint(const uint16_t* T, uint32_t k) { return k ? (uint32_t)T[k - 1u] + (uint32_t)T[k] : 0u; }
ZR_SCALE_FN void zr_scale_midpoints(const uint16_t* T, uint32_t* mid)
{
    for (uint32_t k = 0u; k < 256u; ++k) mid[k] = zr_scale_midpoint(T, k);
}

// The number of k in 1..255 with 2 S >= mid[k] n.  mid ascends strictly, so those k are 1 .. the answer: eight probes find it.
ZR_SCALE_FN uint32_t zr_scale_encode(const uint32_t* mid, uint32_t two_s, uint32_t n)
{
    uint32_t k = 0u;
    for (uint32_t step = 128u; step; step >>= 1)
        if (two_s >= mid[k + step] * n) k += step;       // (k + step <= 255)
    return k;
}

// One block: sum[0..2] = the block's sums of T[R], T[G], T[B], sum[3] = its sum of A, n = its pixels (1 .. 64) -> the output pixel as
// the frame holds one, R in the low byte
ZR_SCALE_FN uint32_t zr_scale_block(const uint32_t* mid, const uint32_t sum[4], uint32_t n)
{
    return zr_scale_encode(mid, 2u * sum[0], n) | (zr_scale_encode(mid, 2u * sum[1], n) << 8) | (zr_scale_encode(mid, 2u * sum[2], n) << 16) |
           (((2u * sum[3] + n) / (2u * n)) << 24);
}

// The host statement of the filter: src is width x height RGBA8, row-major; dst holds ceil(width / s) x ceil(height / s).  Reads nothing
// beyond src[width * height * 4) and writes nothing beyond dst[Wd * Hd * 4).
static inline void zr_scale_frame(const uint8_t* src, uint32_t width, uint32_t height, uint32_t s, uint8_t* dst)
{
    uint32_t mid[256];
    zr_scale_midpoints(kZrScaleT, mid);
    const uint32_t Wd = zr_scale_extent(width, s), Hd = zr_scale_extent(height, s);
    for (uint32_t Y = 0; Y < Hd; ++Y)
        for (uint32_t X = 0; X < Wd; ++X) {
            const uint32_t x1 = (X + 1u) * s < width ? (X + 1u) * s : width, y1 = (Y + 1u) * s < height ? (Y + 1u) * s : height;
            uint32_t sum[4] = { 0u, 0u, 0u, 0u };
            for (uint32_t y = Y * s; y < y1; ++y)
                for (uint32_t x = X * s; x < x1; ++x) {
                    const uint8_t* p = src + ((size_t)y * width + x) * 4u;
                    sum[0] += kZrScaleT[p[0]]; sum[1] += kZrScaleT[p[1]]; sum[2] += kZrScaleT[p[2]]; sum[3] += p[3];
                }
            const uint32_t px = zr_scale_block(mid, sum, (x1 - X * s) * (y1 - Y * s));
            uint8_t* q = dst + ((size_t)Y * Wd + X) * 4u;
            q[0] = (uint8_t)px; q[1] = (uint8_t)(px >> 8); q[2] = (uint8_t)(px >> 16); q[3] = (uint8_t)(px >> 24);
        }
}
