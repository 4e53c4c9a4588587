// highlight_check.cpp — csrc/zr_highlight.h alone, as a stand-alone program (tests/test_highlight_cpu.py compiles it with g++ under the
// address and undefined-behaviour sanitizers and runs it).  Every case of the input file is highlighted twice from exactly-sized heap
// buffers into exactly-sized heap buffers, so one byte read or written beyond any of them stops the program:
//   - by the host statement (zr_hl_frame), whose digest is printed for the test to compare with the reference's;
//   - the way k_highlight_apply goes: the mask as a bit plane of ceil(W / 64) words per row, per 32 x 32 tile the window rows from one
//     or two words (zr_hl_window: under the sanitizer a shift count that is negative or reaches 64 stops the program), dilated along the
//     row and down the rows, then zr_hl_pixel - and the two must agree byte for byte.
// The shift identity of the blend is held to the division for every x in 0 .. 65 025 first.
//   file:  u32 cases, then per case  u32 W, H, radius, 4 bytes outline, 4 bytes fill, W * H * 4 bytes of RGBA8, W * H bytes of mask
//   out:   "case <i> w=<W> h=<H> r=<r> fnv=<16 hex digits>" per case, then "cases <n> failed 0"
#include "zr_highlight.h"

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

// the kernels' way, on the host: what k_highlight_mask leaves (from the byte mask) and what k_highlight_apply makes of it
static void by_windows(const uint8_t* rgba8, const uint8_t* mask, uint32_t W, uint32_t H, const zr_highlight_style* s, uint8_t* dst)
{
    const uint32_t words = zr_hl_row_words(W), r = s->radius, fill = zr_hl_pack(s->fill), outline = zr_hl_pack(s->outline);
    uint64_t* plane = (uint64_t*)malloc((size_t)words * H * sizeof(uint64_t));
    if (!plane) abort();
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t k = 0; k < words; ++k) {
            uint64_t w = 0;
            for (uint32_t b = 0; b < 64u && k * 64u + b < W; ++b) w |= (uint64_t)(mask[(size_t)y * W + k * 64u + b] != 0) << b;
            plane[(size_t)y * words + k] = w;
        }
    for (uint32_t y0 = 0; y0 < H; y0 += kZrHlTile)
        for (uint32_t x0 = 0; x0 < W; x0 += kZrHlTile) {
            uint32_t own[kZrHlTile + 2u * kZrHlRadiusMax], wide[kZrHlTile + 2u * kZrHlRadiusMax];
            const uint32_t rows = kZrHlTile + 2u * r;
            for (uint32_t t = 0; t < rows; ++t) {
                uint64_t win = 0;
                if (y0 + t >= r && y0 + t - r < H) {
                    const uint64_t* row = plane + (size_t)(y0 + t - r) * words;
                    const uint32_t k = x0 >> 6, half = (x0 >> 5) & 1u, klo = half ? k : k - 1u, khi = klo + 1u;
                    const uint64_t lo = (half || r) && klo < words ? row[klo] : 0ull;
                    const uint64_t hi = (!half || r) && khi < words ? row[khi] : 0ull;
                    win = zr_hl_window(lo, hi, half, r);
                }
                own[t] = (uint32_t)(win >> r); wide[t] = (uint32_t)(zr_hl_dilate_row(win, r) >> r);
            }
            for (uint32_t ty = 0; ty < kZrHlTile && y0 + ty < H; ++ty) {
                uint32_t near = 0;
                for (uint32_t i = 0; i <= 2u * r; ++i) near |= wide[ty + i];
                for (uint32_t cx = 0; cx < kZrHlTile && x0 + cx < W; ++cx) {
                    const size_t i = (size_t)(y0 + ty) * W + x0 + cx;
                    uint32_t px;
                    memcpy(&px, rgba8 + i * 4u, 4);      // (little-endian: R in the low byte, as the frame holds a pixel)
                    px = zr_hl_pixel(px, (own[ty + r] >> cx) & 1u, (near >> cx) & 1u, fill, outline);
                    memcpy(dst + i * 4u, &px, 4);
                }
            }
        }
    free(plane);
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: highlight_check cases.bin\n"); return 2; }
    for (uint32_t x = 0; x <= 65025u; ++x)
        if (zr_hl_div255(x) != (x + 127u) / 255u) { fprintf(stderr, "shift identity fails at %u\n", x); return 1; }
    FILE* f = fopen(argv[1], "rb");
    uint32_t cases = 0, failed = 0;
    if (!f || !get32(f, &cases)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    for (uint32_t i = 0; i < cases; ++i) {
        uint32_t W = 0, H = 0;
        zr_highlight_style s;
        memset(&s, 0, sizeof s);
        if (!get32(f, &W) || !get32(f, &H) || !get32(f, &s.radius) || fread(s.outline, 1, 4, f) != 4 || fread(s.fill, 1, 4, f) != 4 || !W || !H || !zr_hl_style_ok(&s)) {
            fprintf(stderr, "case %u: bad header\n", i); return 2;
        }
        const size_t px_bytes = (size_t)W * H * 4u, m_bytes = (size_t)W * H;
        uint8_t* src = (uint8_t*)malloc(px_bytes);
        uint8_t* mask = (uint8_t*)malloc(m_bytes);
        uint8_t* dst = (uint8_t*)malloc(px_bytes);
        uint8_t* dst2 = (uint8_t*)malloc(px_bytes);
        if (!src || !mask || !dst || !dst2 || fread(src, 1, px_bytes, f) != px_bytes || fread(mask, 1, m_bytes, f) != m_bytes) { fprintf(stderr, "case %u: short file\n", i); return 2; }
        memset(dst, 0xA5, px_bytes); memset(dst2, 0x5A, px_bytes);
        zr_hl_frame(src, mask, W, H, &s, dst);
        by_windows(src, mask, W, H, &s, dst2);
        if (memcmp(dst, dst2, px_bytes) != 0) { fprintf(stderr, "case %u: the windows disagree with the rule\n", i); ++failed; }
        printf("case %u w=%u h=%u r=%u fnv=%016llx\n", i, W, H, s.radius, (unsigned long long)fnv1a(dst, px_bytes));
        free(src); free(mask); free(dst); free(dst2);
    }
    fclose(f);
    printf("cases %u failed %u\n", cases, failed);
    return failed ? 1 : 0;
}
