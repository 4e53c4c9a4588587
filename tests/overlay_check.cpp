// overlay_check.cpp — csrc/zr_overlay.h alone, as a stand-alone program (tests/test_overlay_cpu.py compiles it with g++ under the address
// and undefined-behaviour sanitizers, -ffp-contract=off, and runs it).  Every case of the input file is overlaid twice from
// exactly-sized heap buffers into exactly-sized heap buffers, so one byte read or written beyond any of them stops the program:
//   - by the host statement (zr_ov_frame: the walk with its division), whose digest is printed for the test to compare with the
//     reference's;
//   - the way the kernels go: every segment set up into a record and its box of pixels (k_overlay_setup), then per 32 x 32 tile the
//     records whose box reaches it, in index order, over every pixel of the tile by the form without a division (zr_ov_covers) - and
//     the two must agree byte for byte.
// First the bound of zr_overlay.h is asserted at the largest extents zr_create accepts (255 tiles a side, of 32 and of 64 pixels): for
// segments from guard-band corner to guard-band corner, for ends that overshoot it and for a denormal w, the major delta and every
// centre's distance are at most 2^24 and every product of the walk, taken in 128 bits, fits int64; the two forms of the walk agree at
// the ends and in the middle.  Under the sanitizer a signed overflow or a shift count out of range stops the program.
//   file:  u32 cases, then per case  u32 W, H, n, f32 depth_bias, u32 hidden_opacity, 16 f32 PVM, W * H * 4 bytes of RGBA8, W * H f32
//          of depth, n * 32 bytes of segments
//   out:   "case <i> w=<W> h=<H> n=<n> fnv=<16 hex digits>" per case, then "cases <n> failed 0"
#include "zr_overlay.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint64_t fnv1a(const uint8_t* p, size_t n)
{
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}

static bool get(FILE* f, void* v, size_t n) { return fread(v, 1, n, f) == n; }

// the kernels' way, on the host
static void by_tiles(const uint8_t* rgba8, const float* depth, uint32_t W, uint32_t H, const float* pvm, const zr_overlay_segment* seg, uint32_t n,
                     const zr_overlay_style* st, uint8_t* dst)
{
    ZrOvRecord* recs = (ZrOvRecord*)malloc((n ? n : 1u) * sizeof(ZrOvRecord));
    ZrOvBox* boxes = (ZrOvBox*)malloc((n ? n : 1u) * sizeof(ZrOvBox));
    if (!recs || !boxes) abort();
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    for (uint32_t i = 0; i < n; ++i) zr_ov_setup(pvm, hw, hh, W, H, seg[i], &recs[i], &boxes[i]);
    for (uint32_t y0 = 0; y0 < H; y0 += kZrOvTile)
        for (uint32_t x0 = 0; x0 < W; x0 += kZrOvTile) {
            const int32_t tx = (int32_t)(x0 / kZrOvTile), ty = (int32_t)(y0 / kZrOvTile);
            for (uint32_t y = y0; y < y0 + kZrOvTile && y < H; ++y)
                for (uint32_t x = x0; x < x0 + kZrOvTile && x < W; ++x) memcpy(dst + ((size_t)y * W + x) * 4u, rgba8 + ((size_t)y * W + x) * 4u, 4);
            for (uint32_t i = 0; i < n; ++i) {
                const ZrOvBox& B = boxes[i];
                if (recs[i].flags & kZrOvNothing) continue;
                if (!(B.x0 / (int32_t)kZrOvTile <= tx && tx <= B.x1 / (int32_t)kZrOvTile && B.y0 / (int32_t)kZrOvTile <= ty && ty <= B.y1 / (int32_t)kZrOvTile)) continue;
                for (uint32_t y = y0; y < y0 + kZrOvTile && y < H; ++y)
                    for (uint32_t x = x0; x < x0 + kZrOvTile && x < W; ++x) {
                        int32_t k, dm;
                        if (!zr_ov_covers(recs[i], (int32_t)x, (int32_t)y, &k, &dm)) continue;
                        const size_t at = (size_t)y * W + x;
                        uint32_t px;
                        memcpy(&px, dst + at * 4u, 4);      // (little-endian: R in the low byte, as the frame holds a pixel)
                        px = zr_ov_shade(px, depth[at], zr_ov_depth(recs[i], k, dm), recs[i].colour, recs[i].flags, st->depth_bias, st->hidden_opacity);
                        memcpy(dst + at * 4u, &px, 4);
                    }
            }
        }
    free(recs); free(boxes);
}

static bool fits64(__int128 v) { return v >= -((__int128)1 << 62) && v <= ((__int128)1 << 62); }

// the bound at extent E x E: false (with a message) when it does not hold
static bool bound_at(uint32_t E)
{
    // clip = (x, y, z, w) straight from the segment: PVM = identity but for w, which is taken from z (w = z, so z / w = 1 ... any w > 0)
    const float ident[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    const float wz[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0 };      // w = z
    const float g = kZrOvGuard, big = 3.0e38f, tiny = 1.0e-45f;
    struct Try { const float* m; float a[3], b[3]; } tries[] = {
        { ident, { -g, -g, 0.5f }, { g, g, 0.5f } }, { ident, { g, -g, 0.0f }, { -g, g, 1.0f } }, { ident, { -g, 0.3f, 0.5f }, { g, 0.31f, 0.5f } },
        { ident, { 0.3f, g, 0.5f }, { 0.29f, -g, 0.5f } }, { ident, { -100.0f, -90.0f, 0.2f }, { 100.0f, 95.0f, 0.9f } }, { ident, { -big, big, 0.5f }, { big, -big, 0.5f } },
        { ident, { -g, -g, 0.5f }, { -g, g, 0.5f } }, { ident, { -1.0f, -1.0f, 0.5f }, { 1.0f, 1.0f, 0.5f } },
        { wz, { -tiny, tiny, tiny }, { 0.5f, 0.5f, 1.0f } }, { wz, { 1.0f, -1.0f, tiny }, { -1.0f, 1.0f, tiny } }, { wz, { -4.0f, -4.0f, 1.0f }, { 4.0f, 4.0f, 1.0f } },
    };
    const float hw = 0.5f * (float)E, hh = 0.5f * (float)E;
    uint32_t drew = 0;
    for (const Try& t : tries) {
        zr_overlay_segment s;
        memset(&s, 0, sizeof s);
        memcpy(s.a, t.a, sizeof s.a); memcpy(s.b, t.b, sizeof s.b);
        s.rgba[3] = 255;
        ZrOvRecord R;
        ZrOvBox B;
        if (!zr_ov_setup(t.m, hw, hh, E, E, s, &R, &B)) continue;
        ++drew;
        const bool ym = (R.flags & kZrOvYMajor) != 0u;
        const int64_t dM = ym ? (int64_t)R.Yb - R.Ya : (int64_t)R.Xb - R.Xa, dN = ym ? (int64_t)R.Xb - R.Xa : (int64_t)R.Yb - R.Ya;
        const int64_t lim = (int64_t)1 << 24;
        if (!(dM > 0 && dM <= lim && dN <= lim && -dN <= lim && dM >= (dN < 0 ? -dN : dN))) { fprintf(stderr, "extent %u: deltas %lld %lld beyond 2^24\n", E, (long long)dM, (long long)dN); return false; }
        if ((float)(int32_t)dM != (float)dM || (int64_t)(float)dM != dM) { fprintf(stderr, "extent %u: dM not exact in fp32\n", E); return false; }
        const int32_t m0 = ym ? B.y0 : B.x0, m1 = ym ? B.y1 : B.x1;
        const int32_t at[3] = { m0, m0 + (m1 - m0) / 2, m1 };
        for (int32_t m : at) {
            const __int128 Ma = ym ? R.Ya : R.Xa, Na = ym ? R.Xa : R.Ya, k = (__int128)(256 * m + 128) - Ma;
            if (k < 0 || k >= dM || k > lim) { fprintf(stderr, "extent %u: centre distance out of range\n", E); return false; }
            if ((int64_t)(float)(int64_t)k != (int64_t)k) { fprintf(stderr, "extent %u: k not exact in fp32\n", E); return false; }
            const __int128 N = 2 * k * dN + dM, D = 2 * (__int128)dM;
            int32_t kk, dm;
            const int32_t c = zr_ov_walk(R, m, &kk, &dm);
            const __int128 lo = ((__int128)256 * c - Na) * D;
            if (!fits64(N) || !fits64(D) || !fits64(lo) || !fits64(lo + 256 * D)) { fprintf(stderr, "extent %u: a product leaves int64\n", E); return false; }
            int32_t k2, dm2;
            const int32_t x = ym ? c : m, y = ym ? m : c;
            if (!zr_ov_covers(R, x, y, &k2, &dm2) || k2 != kk || dm2 != dm) { fprintf(stderr, "extent %u: the two forms of the walk disagree\n", E); return false; }
            if (zr_ov_covers(R, ym ? c + 1 : m, ym ? m : c + 1, &k2, &dm2) || zr_ov_covers(R, ym ? c - 1 : m, ym ? m : c - 1, &k2, &dm2)) {
                fprintf(stderr, "extent %u: two pixels of one column covered\n", E); return false;
            }
            (void)zr_ov_depth(R, kk, dm);
        }
    }
    if (drew < 8u) { fprintf(stderr, "extent %u: only %u of the bound's segments drew\n", E, drew); return false; }
    return true;
}

// "point" / "project" in.bin out.bin: the header's transform (rows of 19 floats: M, p -> 4 floats) or projection (rows of 6 floats:
// clip, hw, hh -> X, Y as int32 words, z) over a table, for the test to hold to the oracle's word for word
static int functions(const char* which, const char* in, const char* out)
{
    const bool point = strcmp(which, "point") == 0;
    const size_t nin = point ? 19u : 6u, nout = point ? 4u : 3u;
    FILE* f = fopen(in, "rb");
    FILE* g = fopen(out, "wb");
    if (!f || !g) return 2;
    float row[19];
    while (get(f, row, nin * 4u)) {
        uint32_t w[4] = { 0, 0, 0, 0 };
        if (point) {
            const ZrOvVec4 r = zr_ov_point(row, row + 16);
            memcpy(w, &r, 16);
        } else {
            ZrOvVec4 c;
            memcpy(&c, row, 16);
            int32_t X, Y;
            float z;
            zr_ov_project(c, row[4], row[5], &X, &Y, &z);
            w[0] = (uint32_t)X; w[1] = (uint32_t)Y; memcpy(&w[2], &z, 4);
        }
        if (fwrite(w, 4, nout, g) != nout) return 2;
    }
    fclose(f);
    return fclose(g) == 0 ? 0 : 2;
}

int main(int argc, char** argv)
{
    if (argc == 4 && (strcmp(argv[1], "point") == 0 || strcmp(argv[1], "project") == 0)) return functions(argv[1], argv[2], argv[3]);
    if (argc != 2) { fprintf(stderr, "usage: overlay_check cases.bin | overlay_check point|project in.bin out.bin\n"); return 2; }
    if (!bound_at(255u * 32u) || !bound_at(255u * 64u) || !bound_at(66u)) return 1;
    FILE* f = fopen(argv[1], "rb");
    uint32_t cases = 0, failed = 0;
    if (!f || !get(f, &cases, 4)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    for (uint32_t i = 0; i < cases; ++i) {
        uint32_t W = 0, H = 0, n = 0;
        zr_overlay_style st;
        float pvm[16];
        memset(&st, 0, sizeof st);
        if (!get(f, &W, 4) || !get(f, &H, 4) || !get(f, &n, 4) || !get(f, &st.depth_bias, 4) || !get(f, &st.hidden_opacity, 4) || !get(f, pvm, sizeof pvm) || !W || !H ||
            n > ZR_OVERLAY_MAX_SEGMENTS || !zr_ov_style_ok(&st)) {
            fprintf(stderr, "case %u: bad header\n", i); return 2;
        }
        const size_t px_bytes = (size_t)W * H * 4u, d_bytes = (size_t)W * H * sizeof(float), s_bytes = (size_t)n * sizeof(zr_overlay_segment);
        uint8_t* src = (uint8_t*)malloc(px_bytes);
        float* depth = (float*)malloc(d_bytes);
        zr_overlay_segment* seg = (zr_overlay_segment*)malloc(s_bytes ? s_bytes : 1u);
        uint8_t* dst = (uint8_t*)malloc(px_bytes);
        uint8_t* dst2 = (uint8_t*)malloc(px_bytes);
        if (!src || !depth || !seg || !dst || !dst2 || !get(f, src, px_bytes) || !get(f, depth, d_bytes) || (s_bytes && !get(f, seg, s_bytes))) {
            fprintf(stderr, "case %u: short file\n", i); return 2;
        }
        for (uint32_t k = 0; k < n; ++k) if (!zr_ov_flags_ok(seg[k].flags)) { fprintf(stderr, "case %u: bad flags\n", i); return 2; }
        memset(dst, 0xA5, px_bytes); memset(dst2, 0x5A, px_bytes);
        zr_ov_frame(src, depth, W, H, pvm, seg, n, &st, dst);
        by_tiles(src, depth, W, H, pvm, seg, n, &st, dst2);
        if (memcmp(dst, dst2, px_bytes) != 0) { fprintf(stderr, "case %u: the tiles' way disagrees with the walk\n", i); ++failed; }
        printf("case %u w=%u h=%u n=%u fnv=%016llx\n", i, W, H, n, (unsigned long long)fnv1a(dst, px_bytes));
        free(src); free(depth); free(seg); free(dst); free(dst2);
    }
    fclose(f);
    printf("cases %u failed %u\n", cases, failed);
    return failed ? 1 : 0;
}
