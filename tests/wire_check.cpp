// wire_check.cpp — csrc/zr_wire.h alone, as a stand-alone program under the address and undefined-behaviour sanitizers
// (tests/test_wire_cpu.py builds and runs it): the style check, zr_wire_frame's bounds - every array is a heap block of exactly the
// size the statement may touch, on 1 x 1, 1 x N and N x 1 frames among others - the edge order, and dst == blend only where the rule
// says so.  Prints "wire_check failed <n>" last; exits non-zero when n > 0.
#include "zr_wire.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static int failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failed; } } while (0)

// (sx w, sy w, w) in pixels of a W x H frame -> clip space
static void clip(float* c, double sx, double sy, double w, uint32_t W, uint32_t H)
{
    c[0] = (float)((2.0 * sx / W - 1.0) * w); c[1] = (float)((2.0 * sy / H - 1.0) * w); c[2] = (float)w;
}

static void style_check()
{
    zr_wire_style s = zr_wire_style_default();
    CHECK(zr_wire_style_ok(&s) && s.width_256 == 256u && s.flags == 0u && s.rgba[3] == 255u && s.rgba[0] == 0u);
    s.width_256 = 0u; CHECK(!zr_wire_style_ok(&s));
    s.width_256 = 1u; CHECK(zr_wire_style_ok(&s));
    s.width_256 = 4096u; CHECK(zr_wire_style_ok(&s));
    s.width_256 = 4097u; CHECK(!zr_wire_style_ok(&s));
    s.width_256 = 256u; s.flags = ZR_WIRE_SELECTED; CHECK(zr_wire_style_ok(&s));
    s.flags = 2u; CHECK(!zr_wire_style_ok(&s));
    s.flags = 0x80000000u; CHECK(!zr_wire_style_ok(&s));
    s.flags = 0u; s.reserved = 1u; CHECK(!zr_wire_style_ok(&s));
}

// Each edge alone brings its own pixels: a triangle whose edges are the lines x = 2 (0-1), y = 3 (1-2) and the diagonal (2-0)
static void edge_order()
{
    const uint32_t W = 16, H = 16;
    float c[9];
    clip(c, 2.0, 12.0, 1.0, W, H); clip(c + 3, 2.0, 3.0, 2.0, W, H); clip(c + 6, 11.0, 3.0, 0.5, W, H);
    const ZrWireH h0 = zr_wire_corner(c[0], c[1], c[2], 8.0, 8.0), h1 = zr_wire_corner(c[3], c[4], c[5], 8.0, 8.0), h2 = zr_wire_corner(c[6], c[7], c[8], 8.0, 8.0);
    CHECK(h1.x == 4.0 && h1.y == 6.0 && h1.w == 2.0);                       // homogeneous: (2, 3) times w
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const double px = x + 0.5, py = y + 0.5;
            const bool e01 = zr_wire_edge(h0, h1, px, py, 0.25), e12 = zr_wire_edge(h1, h2, px, py, 0.25), e20 = zr_wire_edge(h2, h0, px, py, 0.25);
            CHECK(e01 == (x == 1 || x == 2));                               // |x + 0.5 - 2| <= 0.5: the tie on both sides is on
            CHECK(e12 == (y == 2 || y == 3));
            const double d = (px + py - 14.0);                              // the diagonal is x + y = 14; distance |d| / sqrt 2
            CHECK(e20 == (d * d <= 0.5));
            CHECK(zr_wire_on(c, 8.0, 8.0, x, y, 256u) == (e01 || e12 || e20));
            // the line's orientation does not matter
            CHECK(zr_wire_edge(h1, h0, px, py, 0.25) == e01);
        }
    // coincident corners: no wire from that edge, NaN: false
    CHECK(!zr_wire_edge(h0, h0, 2.5, 2.5, 1e30));
    ZrWireH n = h0; n.x = std::numeric_limits<double>::quiet_NaN();
    CHECK(!zr_wire_edge(n, h1, 2.5, 2.5, 1e30) && !zr_wire_edge(h1, n, 2.5, 2.5, 1e30));
    // behind the eye: the same line
    float b[9]; memcpy(b, c, sizeof b);
    clip(b, 2.0, 12.0, -1.0, W, H);
    for (uint32_t x = 0; x < W; ++x) CHECK(zr_wire_edge(zr_wire_corner(b[0], b[1], b[2], 8.0, 8.0), h1, x + 0.5, 5.5, 0.25) == (x == 1 || x == 2));
}

// One frame through zr_wire_frame with exactly-sized heap blocks, against the rule applied pixel by pixel
static void frame_check(uint32_t W, uint32_t H, uint32_t n_prims, uint32_t width_256, uint32_t flags, bool with_selected, unsigned seed)
{
    const size_t px = (size_t)W * H;
    uint8_t* img = (uint8_t*)std::malloc(px * 4); uint8_t* dst = (uint8_t*)std::malloc(px * 4);
    uint32_t* prim = (uint32_t*)std::malloc(px * 4);
    float* cor = n_prims ? (float*)std::malloc((size_t)n_prims * 9 * sizeof(float)) : nullptr;
    uint8_t* sel = with_selected && n_prims ? (uint8_t*)std::malloc(n_prims) : nullptr;
    std::srand(seed);
    for (size_t i = 0; i < px * 4; ++i) img[i] = (uint8_t)std::rand();
    for (size_t i = 0; i < px; ++i) { const int r = std::rand() % 8; prim[i] = r == 0 ? 0xFFFFFFFFu : r == 1 ? n_prims : (n_prims ? (uint32_t)std::rand() % n_prims : 7u); }
    for (uint32_t k = 0; k < n_prims; ++k)
        for (int v = 0; v < 3; ++v)
            clip(cor + (size_t)k * 9 + v * 3, (std::rand() % 1000) / 1000.0 * W, (std::rand() % 1000) / 1000.0 * H, (v == 2 && k % 3 == 1 ? -1.0 : 1.0) * (0.5 + (std::rand() % 8) / 4.0), W, H);
    for (uint32_t k = 0; sel && k < n_prims; ++k) sel[k] = (uint8_t)(std::rand() % 2 ? std::rand() % 255 + 1 : 0);
    zr_wire_style s = zr_wire_style_default();
    s.rgba[0] = 200; s.rgba[1] = 10; s.rgba[2] = 90; s.rgba[3] = 180; s.width_256 = width_256; s.flags = flags;
    zr_wire_frame(img, prim, W, H, cor, n_prims, sel, &s, dst);
    const uint32_t colour = zr_hl_pack(s.rgba);
    size_t on = 0;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            uint32_t p; memcpy(&p, img + i * 4, 4);
            const bool cand = prim[i] < n_prims && (!(flags & ZR_WIRE_SELECTED) || !sel || sel[prim[i]]);
            const bool wire = cand && zr_wire_on(cor + (size_t)prim[i] * 9, 0.5 * W, 0.5 * H, x, y, width_256);
            const uint32_t want = wire ? zr_hl_blend_px(p, colour) : p;
            uint32_t got; memcpy(&got, dst + i * 4, 4);
            CHECK(got == want);
            CHECK((got >> 24) == (p >> 24));
            on += wire;
        }
    if (W * H >= 256u && n_prims && width_256 == 256u && !(flags & ZR_WIRE_SELECTED)) CHECK(on > 0 && on < px);      // (both verdicts occur)
    std::free(img); std::free(dst); std::free(prim); std::free(cor); std::free(sel);
}

int main()
{
    style_check();
    edge_order();
    const uint32_t extents[][2] = { { 1, 1 }, { 1, 13 }, { 13, 1 }, { 2, 2 }, { 33, 9 }, { 16, 16 } };
    unsigned seed = 1;
    for (const auto& e : extents)
        for (uint32_t width : { 1u, 256u, 1024u, 4096u }) {
            frame_check(e[0], e[1], 5, width, 0u, false, seed++);
            frame_check(e[0], e[1], 5, width, ZR_WIRE_SELECTED, true, seed++);
            frame_check(e[0], e[1], 3, width, ZR_WIRE_SELECTED, false, seed++);
            frame_check(e[0], e[1], 0, width, 0u, false, seed++);
        }
    std::printf("wire_check failed %d\n", failed);
    return failed ? 1 : 0;
}
