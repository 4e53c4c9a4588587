// frame_scale_check.cpp — csrc/zr_scale.h alone, as a stand-alone program (tests/test_frame_scale_cpu.py compiles it with g++ under the
// address and undefined-behaviour sanitizers and runs it): every case of the input file is filtered from an exactly-sized heap buffer into
// an exactly-sized heap buffer, so one byte read or written beyond either stops the program, and a digest of the result is printed for
// the test to compare with the reference's.
//   file:  u32 cases, then per case  u32 W, H, s  and W * H * 4 bytes of RGBA8
//   out:   "case <i> w=<W> h=<H> s=<s> wd=<Wd> hd=<Hd> fnv=<16 hex digits>" per case, then "cases <n> failed 0"
#include "zr_scale.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint64_t fnv1a(const uint8_t* p, size_t n)
{
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}

static bool get32(FILE* f, uint32_t* v)
{
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    *v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: frame_scale_check cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    uint32_t cases = 0;
    if (!f || !get32(f, &cases)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    // the midpoints ascend strictly, which the eight probes of zr_scale_encode rest on
    uint32_t mid[256];
    zr_scale_midpoints(kZrScaleT, mid);
    for (uint32_t k = 2; k < 256u; ++k)
        if (mid[k] <= mid[k - 1u]) { fprintf(stderr, "midpoint %u does not ascend\n", k); return 1; }
    for (uint32_t i = 0; i < cases; ++i) {
        uint32_t W = 0, H = 0, s = 0;
        if (!get32(f, &W) || !get32(f, &H) || !get32(f, &s) || !W || !H || s < 1u || s > kZrScaleMax) { fprintf(stderr, "case %u: bad header\n", i); return 2; }
        const size_t in_bytes = (size_t)W * H * 4u, out_bytes = (size_t)zr_scale_extent(W, s) * zr_scale_extent(H, s) * 4u;
        uint8_t* src = (uint8_t*)malloc(in_bytes);
        uint8_t* dst = (uint8_t*)malloc(out_bytes);
        if (!src || !dst || fread(src, 1, in_bytes, f) != in_bytes) { fprintf(stderr, "case %u: short file\n", i); return 2; }
        memset(dst, 0xA5, out_bytes);
        zr_scale_frame(src, W, H, s, dst);
        printf("case %u w=%u h=%u s=%u wd=%u hd=%u fnv=%016llx\n", i, W, H, s, zr_scale_extent(W, s), zr_scale_extent(H, s), (unsigned long long)fnv1a(dst, out_bytes));
        free(src); free(dst);
    }
    fclose(f);
    printf("cases %u failed 0\n", cases);
    return 0;
}
