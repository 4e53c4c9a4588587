// zr_srgb.h — the host's sRGB encode (what every mip chain built on the CPU goes through) and the table that lets a kernel give the
// same byte without a pow of its own.  Plain C++, no HIP: a stand-alone program can include it (tests/test_texture_update_cpu.py does).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

static inline uint8_t srgb_encode8(float l)
{
    double x = (double)l;
    if (!(x > 0.0)) x = 0.0;
    if (x > 1.0) x = 1.0;
    double s = (x <= 0.0031308) ? 12.92 * x : 1.055 * pow(x, 1.0 / 2.4) - 0.055;
    return (uint8_t)floor(s * 255.0 + 0.5);
}

// thr[k], k = 1 .. 255: the least float that srgb_encode8 maps to k or more, found by bisection over the bit patterns of [0, 1] (for
// floats that are not negative, the order of the patterns is the order of the values).  thr[0] = -inf.  Where srgb_encode8 is monotone
// - the CPU test sweeps it - the number of k with v >= thr[k] is srgb_encode8(v) for every float v, NaN included (it compares false
// everywhere, and the function maps it to 0).  A device pow need not land on the same side of every rounding threshold; a comparison does.
static inline void zr_srgb_thresholds(float thr[256])
{
    thr[0] = -INFINITY;
    for (uint32_t k = 1; k < 256u; ++k) {
        uint32_t lo = 0u, hi = 0x3F800000u;        // encode(0.0f) = 0 < k <= 255 = encode(1.0f)
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            float f; memcpy(&f, &mid, 4);
            if (srgb_encode8(f) >= k) hi = mid; else lo = mid;
        }
        memcpy(&thr[k], &hi, 4);
    }
}
