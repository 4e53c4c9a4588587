// zr_lighting.hip — the deferred-lighting pass (ZE:3531-3540): k_lighting = BaseLighting.frag per pixel (PCF 5x5, per-tile light list,
// ambient, cubemap IBL, gamma, debug views 0-8), k_gbuffer_vis = the GBufferVis mosaic of view 9.
#include "zr_dev.h"
#include "zr_surface.h"
#include "zr_shade.h"

// A pixel nothing was drawn to: every target's clear value (ZE:3427-3433)
__device__ __forceinline__ bool light_pixel_empty(uint32_t sc, uint32_t A, uint32_t B, uint32_t Cc, uint2 D)
{
    return sc == 0xFF000000u && A == 0u && B == 0xFF000000u && Cc == 0xFF000000u && D.x == 0u && D.y == 0x3C000000u;
}

// The per-pixel steps k_lighting and k_lighting_rest share.  light_decode: the GBuffer's words as the shader's inputs (u8 / u10: the LDS
// copies of c / 255 and c / 1023).  light_compose: FinalColor, gamma, the debug-view switch, packed RGBA8.  (What every path
// ends with, light_emit, is k_forward's too: zr_shade.h.)
struct LitPixel { zf3 BaseColor, Normal, N, Pw; float Metallic, Roughness, AO, Mask; };
__device__ __forceinline__ LitPixel light_decode(const float* u8, const float* u10, uint32_t sc, uint32_t A, uint32_t B, uint32_t Cc, uint2 D)
{
    LitPixel q;
    q.BaseColor = zr3(u8[Cc & 255u], u8[(Cc >> 8) & 255u], u8[(Cc >> 16) & 255u]);
    q.Metallic = zr_saturate(u8[B & 255u]);
    q.Roughness = zr_saturate(u8[(B >> 16) & 255u]);
    q.Normal = zr3(__builtin_fmaf(u10[(A >> 20) & 1023u], 2.0f, -1.0f), __builtin_fmaf(u10[(A >> 10) & 1023u], 2.0f, -1.0f),
                   __builtin_fmaf(u10[A & 1023u], 2.0f, -1.0f));
    q.AO = zr_saturate(u8[Cc >> 24]);
    q.Mask = u8[sc >> 24];
    q.Roughness = __builtin_fmaxf(0.01f, q.Roughness);
    q.N = zr_normalize(q.Normal);
    q.Pw = zr3(f16_to_f32_hw(D.x & 0xFFFFu), f16_to_f32_hw(D.x >> 16), f16_to_f32_hw(D.y & 0xFFFFu));
    return q;
}
__device__ __forceinline__ uint32_t light_compose(const ZrLightParams& L, const LitPixel& q, zf3 Direct, zf3 Indirect, zf3 RefC, float ShadowFactor, int px, int py)
{
    zf3 Final = ((Direct + Indirect) + RefC) * q.Mask;
    Final = gamma3(Final);
    zf3 o;
    switch (L.debug_view) {
    case 0: o = Final; break;
    case 1: o = gamma3(q.BaseColor); break;
    case 2: o = zr3(q.Metallic, q.Metallic, q.Metallic); break;
    case 3: o = zr3(q.Roughness, q.Roughness, q.Roughness); break;
    case 4: o = q.Normal; break;
    case 5: o = zr3(q.AO, q.AO, q.AO); break;
    case 7: o = RefC; break;
    case 8: o = zr3(ShadowFactor, ShadowFactor, ShadowFactor); break;
    case 9: o = Final; break;       // GBufferVis: k_gbuffer_vis then overwrites the eight mosaic cells
    case 6: {   // fragColor of the full-screen quad: Background.vert:10-17 vertex colours over its two triangles
        const float u = ((float)px + 0.5f) / (float)L.W, v = ((float)py + 0.5f) / (float)L.H;
        o = v >= u ? zr3(1.0f - v, u, v - u) : zr3(1.0f - u, v, u - v);
        break;
    }
    default: o = Final * ShadowFactor; break;
    }
    return pack_rgb8(o);
}
// The clear of the next frame's shadow pass (depth 1.0, ZE:3248), a slice per workgroup of the lighting launch: saves a launch
template <int TB>
__device__ __forceinline__ void light_clear_next_slice(const ZrLightParams& L)
{
    if (!L.clear_next) return;
    const uint32_t per = (L.clear_n + gridDim.x - 1u) / gridDim.x, b = blockIdx.x * per;
    for (uint32_t i = threadIdx.x; i < per && b + i < L.clear_n; i += (uint32_t)TB) L.clear_next[b + i] = 0x3F800000u;
}

// BaseLighting.frag:147-254 for every pixel of the owned tiles (the full-screen quad of ZE:3531-3540)
// MODE (ZrLightMode): FILL also stores the pixel's standing terms - Direct after the directional lights, ShadowFactor, RefC, exact fp32 - into
// the context's plane; KEPT loads them instead of running shade_standing (no PCF, no directional BxDF, no cubemap) and goes on as ever: the
// point lights, Indirect, compose, gamma, the debug views.  Pixels that take the empty-pixel shortcut touch the plane in neither mode.
template <bool LIGHT_LIST, bool BACKGROUND, int TB, int PPT, uint32_t MODE>      // PPT: pixels per thread, 4 or 1 (as in k_resolve_gbuffer)
// (compiled for exactly ZR_LIGHT_WAVES waves per SIMD; left to itself the allocator takes 127 registers.  Rounds 4 - 5 ran it at 4 waves
// (97 VGPRs): beside a camera lane that filled the whole period, a fifth wave cost that lane more than it gave this pass.  With that lane's
// scans and index passes gone (round 6) the frame's period was THIS lane's, and the fifth wave paid: 4 / 5 / 6 waves 5 548 / 5 670 / 5 420
// Mpixel/s.  On a frame that keeps its camera pass the kernel runs alone, and a sixth pays: 16 770 / 17 470 / 19 363, the moving-camera
// loop, where the lane is still there, the same within its margin.  The KEPT variant is compiled for
// ZR_LIGHT_KEPT_WAVES: it needs far fewer registers.)
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(MODE == ZR_LIGHT_KEPT ? ZR_LIGHT_KEPT_WAVES : ZR_LIGHT_WAVES, MODE == ZR_LIGHT_KEPT ? ZR_LIGHT_KEPT_WAVES : ZR_LIGHT_WAVES))) void k_lighting(ZrLightParams L, const XkView* __restrict__ view,
                                                  const uint32_t* __restrict__ owned_tiles, GBufferPtrs G,
                                                  const float* __restrict__ shadowmap, CubeDesc C,
                                                  const float* __restrict__ srgb_lut, const float* __restrict__ unorm_lut,
                                                  uint32_t* __restrict__ out, float4* __restrict__ plane, float4* __restrict__ rest)
{
    // UNORM loads are IEEE quotients c / 255 and c / 1023: 14 per pixel, served from an LDS copy of the host-built table
    __shared__ float tl[512];            // [0, 256) sRGB decode (24 cubemap fetches per pixel), [256, 512) c / 255: tex_decode's layout
    __shared__ float u10[1024];
    float* const slut = tl; float* const u8 = tl + 256;
    constexpr uint32_t T = TILE_PIX / (uint32_t)PPT, PARTS = T / (uint32_t)TB, WAVES = (uint32_t)TB / 64u;
    const uint32_t tid = threadIdx.x + (blockIdx.x % PARTS) * (uint32_t)TB;      // the thread's place among the tile's T
    const uint32_t tile_slot = blockIdx.x / PARTS;
    for (uint32_t i = threadIdx.x; i < 256u; i += (uint32_t)TB) { u8[i] = unorm_lut[i]; slut[i] = srgb_lut[i]; }
    for (uint32_t i = threadIdx.x; i < 1024u; i += (uint32_t)TB) u10[i] = unorm_lut[256u + i];
    __syncthreads();
    light_clear_next_slice<TB>(L);
    const uint32_t tile = owned_tiles[tile_slot];
    const int tx0 = (int)(tile % L.tiles_x) * TILE, ty0 = (int)(tile / L.tiles_x) * TILE;
    const zf3 cam = zr3(view->CameraInfo[0], view->CameraInfo[1], view->CameraInfo[2]);
    const uint32_t nDir = (uint32_t)view->LightsCount[0], nPoint = (uint32_t)view->LightsCount[1];
    const float maxmips = (float)(uint32_t)view->LightsCount[3];
    const float dxy = 1.5f * 1.0f / (float)L.SD;

    // Tile light list (LIGHT_LIST: four or more point lights): a light whose sphere of influence misses the bounding box of the tile's world
    // positions would be skipped by every pixel's own exact test below (|lp - P| >= the box distance per axis, and the squared
    // sums are monotonic), so it is dropped for the whole tile.  The list is a bitmask, walked in ascending order: the
    // accumulation order over lights is unchanged.  Pixels with Mask = 0 do not count: their colour is (...) * 0 -> stored 0.
    __shared__ float bbp[LIGHT_LIST ? WAVES : 1][6];
    __shared__ uint32_t lmask[LIGHT_LIST ? XK_MAX_POINT_LIGHTS_NUM / 32 : 1];
    constexpr bool use_mask = LIGHT_LIST;
    // The fill also records, per wave (one pixel per thread: 64 consecutive pixels of the tile), that box and which of its pixels hold every
    // target's clear value (ZrRestRecord): the GBuffer stands for the whole rest, and the resting frame's launch (k_lighting_rest) reads
    // the records instead of the GBuffer.
    constexpr bool RECORDS = MODE == ZR_LIGHT_FILL && PPT == 1;
    if constexpr (LIGHT_LIST || RECORDS) {
        float lo[3] = { __builtin_inff(), __builtin_inff(), __builtin_inff() }, hi[3] = { -__builtin_inff(), -__builtin_inff(), -__builtin_inff() };
        bool odd = false;                    // a non-finite position: keep every light
        bool empty = false;
        for (uint32_t i = tid; i < TILE_PIX; i += T) {
            const int px = tx0 + (int)(i & (TILE - 1)), py = ty0 + (int)(i / TILE);
            if (px >= (int)L.W || py >= (int)L.H) continue;
            const size_t p = (size_t)py * L.W + (size_t)px;
            if constexpr (RECORDS) empty = light_pixel_empty(G.scene_color[p], G.gA[p], G.gB[p], G.gC[p], G.gD[p]);
            if ((G.scene_color[p] >> 24) == 0u) continue;
            const uint2 D = G.gD[p];
            const float q[3] = { f16_to_f32_hw(D.x & 0xFFFFu), f16_to_f32_hw(D.x >> 16), f16_to_f32_hw(D.y & 0xFFFFu) };
            for (int a = 0; a < 3; ++a) {
                if (!(__builtin_fabsf(q[a]) <= 3.402823466e38f)) odd = true;
                lo[a] = __builtin_fminf(lo[a], q[a]); hi[a] = __builtin_fmaxf(hi[a], q[a]);
            }
        }
        for (int a = 0; a < 3; ++a) { lo[a] = wave_fmin(lo[a]); hi[a] = wave_fmax(hi[a]); }
        const bool wodd = __ballot(odd) != 0ull;
        if constexpr (RECORDS) {
            const unsigned long long em = __ballot(empty);
            if (rest != nullptr && (threadIdx.x & 63u) == 0u) {
                ZrRestRecord* r = (ZrRestRecord*)(rest + ZR_REST_SLOT) + ((size_t)tile_slot * ZR_REST_RECORDS_PER_TILE + (tid >> 6));
                for (int a = 0; a < 3; ++a) { r->lo[a] = wodd ? -__builtin_inff() : lo[a]; r->hi[a] = wodd ? __builtin_inff() : hi[a]; }
                r->empty[0] = (uint32_t)em; r->empty[1] = (uint32_t)(em >> 32);
            }
        }
        if constexpr (LIGHT_LIST) {
            if ((threadIdx.x & 63u) == 0u) {
                float* o = bbp[threadIdx.x >> 6];
                o[0] = wodd ? -__builtin_inff() : lo[0]; o[1] = wodd ? -__builtin_inff() : lo[1]; o[2] = wodd ? -__builtin_inff() : lo[2];
                o[3] = wodd ? __builtin_inff() : hi[0]; o[4] = wodd ? __builtin_inff() : hi[1]; o[5] = wodd ? __builtin_inff() : hi[2];
            }
            for (uint32_t i = threadIdx.x; i < XK_MAX_POINT_LIGHTS_NUM / 32; i += (uint32_t)TB) lmask[i] = 0u;
            __syncthreads();
            float blo[3], bhi[3];
            for (int a = 0; a < 3; ++a) {
                blo[a] = bbp[0][a]; bhi[a] = bbp[0][3 + a];
                for (uint32_t w = 1; w < WAVES; ++w) { blo[a] = __builtin_fminf(blo[a], bbp[w][a]); bhi[a] = __builtin_fmaxf(bhi[a], bbp[w][3 + a]); }
            }
            for (uint32_t li = threadIdx.x; li < nPoint; li += (uint32_t)TB)
                if (light_listed(ViewLight{ &view->PointLights[li] }, blo, bhi)) atomicOr(&lmask[li >> 5], 1u << (li & 31u));
            __syncthreads();
        }
    }

    for (uint32_t i = tid; i < TILE_PIX; i += T) {
        const int px = tx0 + (int)(i & (TILE - 1)), py = ty0 + (int)(i / TILE);
        if (px >= (int)L.W || py >= (int)L.H) continue;
        const size_t p = (size_t)py * L.W + (size_t)px;
        const uint32_t sc = G.scene_color[p], A = G.gA[p], B = G.gB[p], Cc = G.gC[p];
        const uint2 D = G.gD[p];
        // A pixel nothing was drawn to holds the clear values of every target (ZE:3427-3433), so the shader computes the same
        // colour for all of them: it was computed once (zr_launch_lighting's one-pixel pre-launch of this very kernel).
        // (light_pixel_empty() spelt out: as a call behind the null test it changes the plain instantiations' code)
        if (L.empty_rgba != nullptr && sc == 0xFF000000u && A == 0u && B == 0xFF000000u && Cc == 0xFF000000u && D.x == 0u && D.y == 0x3C000000u) {
            light_emit<BACKGROUND>(L, G, tl, out, *L.empty_rgba, px, py, p, tile_slot, i);
            continue;
        }
        const LitPixel q = light_decode(u8, u10, sc, A, B, Cc, D);
        zf3 Direct, Indirect, RefC; float ShadowFactor;
        if constexpr (MODE == ZR_LIGHT_KEPT) {      // the standing terms as the fill stored them: two 16-byte loads
            const float4 ka = plane[p], kb = plane[(size_t)L.W * L.H + p];
            Direct = zr3(ka.x, ka.y, ka.z); ShadowFactor = ka.w; RefC = zr3(kb.x, kb.y, kb.z);
            shade_points<use_mask>(L, view, lmask, nDir, nPoint, cam, q.BaseColor, q.Metallic, q.Roughness, q.N, q.Pw, Direct);
            Indirect = shade_indirect(q.BaseColor, q.Metallic, q.AO, ShadowFactor);
        } else if constexpr (MODE == ZR_LIGHT_FILL) {
            shade_standing(L, view, shadowmap, C, slut, nDir, maxmips, dxy, cam, q.BaseColor, q.Metallic, q.Roughness, q.N, q.AO, q.Pw, Direct, RefC, ShadowFactor);
            plane[p] = make_float4(Direct.x, Direct.y, Direct.z, ShadowFactor);
            plane[(size_t)L.W * L.H + p] = make_float4(RefC.x, RefC.y, RefC.z, 0.0f);
            shade_points<use_mask>(L, view, lmask, nDir, nPoint, cam, q.BaseColor, q.Metallic, q.Roughness, q.N, q.Pw, Direct);
            Indirect = shade_indirect(q.BaseColor, q.Metallic, q.AO, ShadowFactor);
        } else
            shade_surface<use_mask>(L, view, shadowmap, C, slut, lmask, nDir, nPoint, maxmips, dxy, cam, q.BaseColor, q.Metallic, q.Roughness, q.N, q.AO, q.Pw,
                                    Direct, Indirect, RefC, ShadowFactor);
        light_emit<BACKGROUND>(L, G, tl, out, light_compose(L, q, Direct, Indirect, RefC, ShadowFactor, px, py), px, py, p, tile_slot, i);
    }
}

// The resting frame in one launch: what k_lighting<.., ZR_LIGHT_KEPT> computes, bit for bit, for a frame that uploads nothing and launches
// nothing else ("The schedule").
//  - The moving uniforms - camera position, light counts, the point lights - are the argument R (zr_shade.h, ArgLight).
//  - What the GBuffer decides was recorded by the fill (ZrRestRecord, one per wave): the workgroup merges its waves' boxes (min / max are
//    exact: the tile's list is k_lighting's), each wave tests the lights against the box itself - a ballot, no LDS list, no barrier -
//    and knows its empty pixels without fetching their 24 GBuffer bytes.
//  - The colour of a pixel that holds every target's clear value moves with the point lights, so it is computed here, by the thread that
//    owns the workgroup's first such pixel: that pixel shaded like any other, its standing terms from the slot the fill's one-pixel
//    launch wrote (rest[0], rest[1]) instead of plane[p], parked in LDS behind one barrier whose condition the records make uniform.
//    Every workgroup that holds an empty pixel computes the same colour: none waits for another.
//  - Set-up is by round trips, not by loops of them.  The 1 536 table floats, an LDS copy of the light records and the part's records
//    are all requested before the first of them is waited for.  The part's eight records arrive as ONE dword per lane, laid out so
//    that half a row of 16 lanes holds one field of every record: the box is three DPP steps of min and three of max, the masks are lane
//    reads.  A light's record arrives whole (zr_shade.h, ArgLight): the list's test reads the lane's light from the LDS copy, the light
//    loop by one scalar load of eight dwords.
// One pixel per thread only (the records are per wave of such a kernel); other builds keep the pass that reads XkView.
#if ZR_PIXELS_PER_THREAD == 1
// Of a part's WAVES (at most 8) records a dword per lane: lane 8 f + w of a wave holds field f of record w % WAVES (fields 0 - 2 lo,
// 3 - 5 hi, 6 - 7 empty): the eight lanes of a field are half a DPP row.
template <uint32_t WAVES>
__device__ __forceinline__ uint32_t rest_records_fetch(const float4* __restrict__ rest, uint32_t first_record)
{
    constexpr uint32_t RECW = (uint32_t)(sizeof(ZrRestRecord) / 4u);
    const uint32_t* __restrict__ w = (const uint32_t*)(rest + ZR_REST_SLOT) + (size_t)first_record * RECW;      // (wave-uniform; the lane's offset is 32 bits)
    return w[((threadIdx.x & 7u) % WAVES) * RECW + ((threadIdx.x >> 3) & 7u)];
}
// The steps the three resting kernels share, each spelled once (which test holds which: DESIGN.md App. A, "Resting-frame kernels").
// The 1 536 table floats (k_lighting's tl - sRGB decode, then c / 255: tex_decode's layout - and u10, in one piece): every request is
// issued before the first store waits for one.  k_lighting_rest and k_lighting_stand's control build put more requests between the two.
template <int TB>
__device__ __forceinline__ void rest_tables_request(float (&tv)[1536 / TB], const float* __restrict__ srgb_lut, const float* __restrict__ unorm_lut)
{
#pragma unroll
    for (uint32_t k = 0; k < 1536u / (uint32_t)TB; ++k) { const uint32_t j = threadIdx.x + k * (uint32_t)TB; tv[k] = j < 256u ? srgb_lut[j] : unorm_lut[j - 256u]; }
}
template <int TB>
__device__ __forceinline__ void rest_tables_store(float* tab, const float (&tv)[1536 / TB])
{
#pragma unroll
    for (uint32_t k = 0; k < 1536u / (uint32_t)TB; ++k) tab[threadIdx.x + k * (uint32_t)TB] = tv[k];
}
template <int TB>
__device__ __forceinline__ void rest_tables_load(float* tab, const float* __restrict__ srgb_lut, const float* __restrict__ unorm_lut)
{
    float tv[1536 / TB];
    rest_tables_request<TB>(tv, srgb_lut, unorm_lut);
    rest_tables_store<TB>(tab, tv);
}
// The part's box from its records' dword per lane.  row_shr 1, 2, 4 fold exactly eight lanes into the last of them: lane 8 f + 7 holds
// field f over the records (min / max are exact in any order; the fill's -inf / +inf for a non-finite position pass through as they did)
__device__ __forceinline__ void rest_box_fold(uint32_t rec, float* blo, float* bhi)
{
    int lo, hi;
    { const int idn = 0x7F800000; int r = (int)rec; ZR_DPP_STEP(op_fmin, 0x111, 0xF); ZR_DPP_STEP(op_fmin, 0x112, 0xF); ZR_DPP_STEP(op_fmin, 0x114, 0xF); lo = r; }
    { const int idn = (int)0xFF800000; int r = (int)rec; ZR_DPP_STEP(op_fmax, 0x111, 0xF); ZR_DPP_STEP(op_fmax, 0x112, 0xF); ZR_DPP_STEP(op_fmax, 0x114, 0xF); hi = r; }
    for (int a = 0; a < 3; ++a) { blo[a] = zr_u2f((uint32_t)__builtin_amdgcn_readlane(lo, 8 * a + 7)); bhi[a] = zr_u2f((uint32_t)__builtin_amdgcn_readlane(hi, 8 * (3 + a) + 7)); }
}
// Record w's empty pixels, a bit each: lanes 48 + w and 56 + w hold the two halves
__device__ __forceinline__ unsigned long long rest_mask_of(uint32_t rec, int w)
{
    return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)rec, 48 + w) | (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)rec, 56 + w) << 32;
}
// The part's first empty pixel (thread number, or REST_NONE).  WIDEN: a part that holds one has its box widened to the world origin - the
// empty pixel is shaded at Pw = 0, and the empty colour's settling rests on the box holding it.
constexpr uint32_t REST_NONE = 0xFFFFFFFFu;
template <uint32_t WAVES, bool WIDEN>
__device__ __forceinline__ uint32_t rest_first_empty(uint32_t rec, float* blo, float* bhi)
{
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long nz64 = __ballot(lane >= 48u && (lane & 7u) < WAVES && rec != 0u);
    const uint32_t nz = ((uint32_t)(nz64 >> 48) | (uint32_t)(nz64 >> 56)) & 255u;      // bit w: record w holds an empty pixel
    uint32_t first = REST_NONE;
    if (nz != 0u) {
        const int w0 = __builtin_ctz(nz);
        first = (uint32_t)w0 * 64u + (uint32_t)__builtin_ctzll(rest_mask_of(rec, w0));
        if constexpr (WIDEN)
            for (int a = 0; a < 3; ++a) { blo[a] = __builtin_fminf(blo[a], 0.0f); bhi[a] = __builtin_fmaxf(bhi[a], 0.0f); }
    }
    return first;
}
// What a part decides, the same in every wave that works it out (every operand is): reach = the tile list's ballot over the part's box,
// a lane a light; first = its first empty pixel; settled = no light reaches it and its mark stands.
struct RestDecision { unsigned long long reach; uint32_t first; bool settled; };
template <uint32_t WAVES>
__device__ __forceinline__ RestDecision rest_decide(uint32_t rec, uint32_t mark, const ArgLight& mine_light, uint32_t nPoint, uint32_t gen)
{
    RestDecision d;
    float blo[3], bhi[3];
    rest_box_fold(rec, blo, bhi);
    d.first = rest_first_empty<WAVES, true>(rec, blo, bhi);
    d.reach = __ballot((threadIdx.x & 63u) < nPoint && light_listed(mine_light, blo, bhi));
    d.settled = gen != 0u && d.reach == 0ull && mark == gen;
    return d;
}
// A part's pixels.  What the fill recorded says which are empty (mine: this wave's, a bit per lane); the rest fetch their GBuffer words and
// are shaded as k_lighting<.., ZR_LIGHT_KEPT> shades them, the lights from R, walked by list (USE_LIST) or all of them.  The colour of
// an empty pixel is computed by the thread that owns the part's first (first: its thread number, or REST_NONE) - that pixel shaded like
// any other, its standing terms from the slot the fill's one-pixel launch wrote - and parked in LDS behind one barrier, whose condition
// is the same for every thread of the workgroup.
template <bool USE_LIST, bool BACKGROUND>
__device__ __forceinline__ void rest_shade_part(const ZrLightParams& L, const ZrRestArgs& R, const GBufferPtrs& G, const float* tab, uint32_t* __restrict__ out,
                                                const float4* __restrict__ plane, const float4* __restrict__ rest, unsigned long long list, uint32_t first,
                                                unsigned long long mine, uint32_t tile, uint32_t tile_slot, uint32_t i, uint32_t* empty_px)
{
    const float* const tl = tab; const float* const u8 = tab + 256; const float* const u10 = tab + 512;
    const int tx0 = (int)(tile % L.tiles_x) * TILE, ty0 = (int)(tile / L.tiles_x) * TILE;
    const zf3 cam = zr3(R.cam[0], R.cam[1], R.cam[2]);
    const int px = tx0 + (int)(i & (TILE - 1)), py = ty0 + (int)(i / TILE);
    const bool inside = px < (int)L.W && py < (int)L.H;
    const size_t p = (size_t)py * L.W + (size_t)px;
    const bool is_empty = ((mine >> (threadIdx.x & 63u)) & 1ull) != 0ull, owner = threadIdx.x == first;
    if (inside && (!is_empty || owner)) {
        const uint32_t sc = G.scene_color[p], A = G.gA[p], B = G.gB[p], Cc = G.gC[p];
        const uint2 D = G.gD[p];
        const LitPixel q = light_decode(u8, u10, sc, A, B, Cc, D);
        const float4 ka = owner ? rest[0] : plane[p], kb = owner ? rest[1] : plane[(size_t)L.W * L.H + p];
        zf3 Direct = zr3(ka.x, ka.y, ka.z); const float ShadowFactor = ka.w; const zf3 RefC = zr3(kb.x, kb.y, kb.z);
        shade_points_arg<USE_LIST>(L, R, list, cam, q.BaseColor, q.Metallic, q.Roughness, q.N, q.Pw, Direct);
        const zf3 Indirect = shade_indirect(q.BaseColor, q.Metallic, q.AO, ShadowFactor);
        const uint32_t rgba = light_compose(L, q, Direct, Indirect, RefC, ShadowFactor, px, py);
        if (owner) *empty_px = rgba;
        else light_emit<BACKGROUND>(L, G, tl, out, rgba, px, py, p, tile_slot, i);
    }
    if (first != REST_NONE) {
        __syncthreads();
        if (inside && is_empty) light_emit<BACKGROUND>(L, G, tl, out, *empty_px, px, py, p, tile_slot, i);
    }
}

template <bool LIGHT_LIST, bool BACKGROUND, int TB>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(ZR_LIGHT_KEPT_WAVES, ZR_LIGHT_KEPT_WAVES)))
void k_lighting_rest(ZrLightParams L, ZrRestArgs R, const uint32_t* __restrict__ owned_tiles, GBufferPtrs G, const float* __restrict__ srgb_lut,
                     const float* __restrict__ unorm_lut, uint32_t* __restrict__ out, const float4* __restrict__ plane, const float4* __restrict__ rest)
{
    static_assert(sizeof(ZrLightParams) + sizeof(ZrRestArgs) + sizeof(GBufferPtrs) + 6 * sizeof(void*) + 256 /* the hidden arguments */ < 4096,
                  "k_lighting_rest: the argument block");
    constexpr uint32_t PARTS = TILE_PIX / (uint32_t)TB, WAVES = (uint32_t)TB / 64u;
    static_assert((WAVES <= 8u || !ZR_REST_RECORDS_ONE_TRIP) && 1536u % (uint32_t)TB == 0u, "k_lighting_rest: a part's records are a dword per lane");
    __shared__ float tab[1536];          // rest_tables_load's
    __shared__ uint32_t empty_px;
    __shared__ ZrRestLight lpt[LIGHT_LIST ? ZR_REST_ARG_LIGHTS : 1];      // the light records' LDS copy, for the tile list's test (a lane per light)
    const uint32_t part = blockIdx.x % PARTS, tile_slot = blockIdx.x / PARTS;
    const uint32_t i = threadIdx.x + part * (uint32_t)TB;      // the thread's pixel among the tile's
    const uint32_t first_record = tile_slot * ZR_REST_RECORDS_PER_TILE + part * WAVES;
    uint32_t rec = 0u;
    {   // every load is issued before the first is waited for
        constexpr uint32_t LW = ZR_REST_ARG_LIGHTS * (uint32_t)(sizeof(ZrRestLight) / 4u), NL = LIGHT_LIST ? (LW + (uint32_t)TB - 1u) / (uint32_t)TB : 0u;
        float tv[1536 / TB], lv[NL ? NL : 1u];
        rest_tables_request<TB>(tv, srgb_lut, unorm_lut);
#pragma unroll
        for (uint32_t k = 0; k < NL; ++k) { const uint32_t j = threadIdx.x + k * (uint32_t)TB; lv[k] = ((const float*)R.pt)[LW % (uint32_t)TB == 0u || j < LW ? j : 0u]; }
        if (ZR_REST_RECORDS_ONE_TRIP) rec = rest_records_fetch<WAVES>(rest, first_record);
        rest_tables_store<TB>(tab, tv);
#pragma unroll
        for (uint32_t k = 0; k < NL; ++k) { const uint32_t j = threadIdx.x + k * (uint32_t)TB; if (LW % (uint32_t)TB == 0u || j < LW) ((float*)lpt)[j] = lv[k]; }
    }
    const uint32_t tile = owned_tiles[tile_slot];
    __syncthreads();
    light_clear_next_slice<TB>(L);
    // the workgroup's records: the tile's box, the first empty pixel (thread number, or REST_NONE), this wave's empty pixels
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float blo[3] = { __builtin_inff(), __builtin_inff(), __builtin_inff() }, bhi[3] = { -__builtin_inff(), -__builtin_inff(), -__builtin_inff() };
    uint32_t first = REST_NONE;
    unsigned long long mine = 0ull;
#if ZR_REST_RECORDS_ONE_TRIP
    if constexpr (LIGHT_LIST) rest_box_fold(rec, blo, bhi);
    first = rest_first_empty<WAVES, false>(rec, blo, bhi);
    mine = rest_mask_of(rec, (int)wave);
#else      // (the control build of tests/test_kernel_table_rest_setup.py: a record at a time, a scalar load and a wait each)
    const ZrRestRecord* __restrict__ recs = (const ZrRestRecord*)(rest + ZR_REST_SLOT) + first_record;
#pragma unroll 1      // (unrolled, the eight records' 64 scalar registers spill)
    for (uint32_t w = 0; w < WAVES; ++w) {
        if constexpr (LIGHT_LIST)
            for (int a = 0; a < 3; ++a) { blo[a] = __builtin_fminf(blo[a], recs[w].lo[a]); bhi[a] = __builtin_fmaxf(bhi[a], recs[w].hi[a]); }
        const unsigned long long em = (unsigned long long)recs[w].empty[0] | (unsigned long long)recs[w].empty[1] << 32;
        if (em != 0ull && first == REST_NONE) first = w * 64u + (uint32_t)__builtin_ctzll(em);
        if (w == wave) mine = em;
    }
#endif
    unsigned long long amask = 0ull;      // the tile's light list (at most ZR_REST_ARG_LIGHTS = 64 lights: a lane each)
    if constexpr (LIGHT_LIST) {
        const uint32_t li = threadIdx.x & 63u;
        amask = __ballot(li < R.nPoint && light_listed(ArgLight{ &lpt[li < R.nPoint ? li : 0u] }, blo, bhi));
    }
    rest_shade_part<LIGHT_LIST, BACKGROUND>(L, R, G, tab, out, plane, rest, amask, first, mine, tile, tile_slot, i, &empty_px);
}

// The resting frame's launch on a context whose target only this library writes (zr_settle.h): k_lighting_rest, except that a part no
// point light reaches leaves its pixels as they stand.  On a resting frame only the point lights move: a pixel none of them reaches gets
// the colour the launch before wrote to the same address.  marks[part] == gen says that the part's pixels in the target ARE that colour -
// written by a launch of this generation that found the part out of every light's reach - and the host moves gen on whenever the colour
// or the target's bytes may have changed behind the kernel's back (gen 0: settling is off, nothing is skipped or marked).
//  - reach = the tile list's ballot over the part's box.  The fill's box holds the world origin wherever the part holds an empty pixel
//    (its GBuffer D is the clear value); it is widened to it once more here, since the empty colour's settling rests on it.  reach == 0
//    exactly when every pixel's own test would skip every light; the same ballot is the light loop's list (always built: a lane a light).
//  - The part's records, its mark and the lane's light record (from the argument block, two 16-byte loads) are one trip, and a settled
//    part returns behind it: no table load, no LDS, no barrier.  A part that shades pays a second trip for the tables.
//    (-DZR_STAND_EARLY_EXIT=0: all of it in one trip and the exit behind the barrier - the losing order, DESIGN.md App. A.)
//  - settled is the same for every wave of the workgroup: each reads the same records, the same mark, the same lights.
//  - A part that shades does what k_lighting_rest does, through the same steps (rest_shade_part); behind the set-up's barrier (every wave has read the mark
//    by then) thread 0 sets the mark (reach == 0), takes it back (reach != 0 and it stood) or - the steady state - writes nothing.
#ifndef ZR_STAND_EARLY_EXIT
#define ZR_STAND_EARLY_EXIT 1
#endif
template <bool BACKGROUND, int TB>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(ZR_LIGHT_KEPT_WAVES, ZR_LIGHT_KEPT_WAVES)))
void k_lighting_stand(ZrLightParams L, ZrRestArgs R, const uint32_t* __restrict__ owned_tiles, GBufferPtrs G, const float* __restrict__ srgb_lut,
                      const float* __restrict__ unorm_lut, uint32_t* __restrict__ out, const float4* __restrict__ plane, const float4* __restrict__ rest,
                      uint32_t* marks, uint32_t gen)
{
    static_assert(sizeof(ZrLightParams) + sizeof(ZrRestArgs) + sizeof(GBufferPtrs) + 8 * sizeof(void*) + 256 /* the hidden arguments */ < 4096,
                  "k_lighting_stand: the argument block");
    constexpr uint32_t PARTS = TILE_PIX / (uint32_t)TB, WAVES = (uint32_t)TB / 64u;
    static_assert(WAVES <= 8u && 1536u % (uint32_t)TB == 0u, "k_lighting_stand: a part's records are a dword per lane");
    __shared__ float tab[1536];          // rest_tables_load's
    __shared__ uint32_t empty_px;
    const uint32_t part = blockIdx.x % PARTS, tile_slot = blockIdx.x / PARTS;
    const uint32_t i = threadIdx.x + part * (uint32_t)TB;      // the thread's pixel among the tile's
    const uint32_t lane = threadIdx.x & 63u;
#if !ZR_STAND_EARLY_EXIT
    float tv[1536 / TB];
    rest_tables_request<TB>(tv, srgb_lut, unorm_lut);
#endif
    const uint32_t rec = rest_records_fetch<WAVES>(rest, tile_slot * ZR_REST_RECORDS_PER_TILE + part * WAVES);
    const ZrRestLight* const lights = R.pt;
    const ArgLight mine_light{ &lights[lane < R.nPoint ? lane : 0u] };
    const uint32_t mark = (uint32_t)__builtin_amdgcn_readfirstlane((int)marks[blockIdx.x]);
#if !ZR_STAND_EARLY_EXIT
    rest_tables_store<TB>(tab, tv);
    const uint32_t tile = owned_tiles[tile_slot];
    __syncthreads();
#endif

    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long mine = rest_mask_of(rec, (int)wave);      // this wave's empty pixels
    const RestDecision d = rest_decide<WAVES>(rec, mark, mine_light, R.nPoint, gen);
    if (d.settled) { light_clear_next_slice<TB>(L); return; }

#if ZR_STAND_EARLY_EXIT
    rest_tables_load<TB>(tab, srgb_lut, unorm_lut);
    const uint32_t tile = owned_tiles[tile_slot];
    __syncthreads();
#endif
    // The mark's update: behind the set-up's barrier - every wave of the workgroup has read the mark and decided before it arrives there,
    // so no wave can see this launch's own store and return from a part its siblings shade - and ahead of the pixel, so that nothing of
    // it lives across the shading.  (The next launch is behind the store by stream order.)
    if (gen != 0u && threadIdx.x == 0u) {
        if (d.reach == 0ull) marks[blockIdx.x] = gen;            // (it did not stand, or the part had returned)
        else if (mark == gen) marks[blockIdx.x] = 0u;
    }
    light_clear_next_slice<TB>(L);
    rest_shade_part<true, BACKGROUND>(L, R, G, tab, out, plane, rest, d.reach, d.first, mine, tile, tile_slot, i, &empty_px);
}
// k_lighting_stand with the part's decision made ONCE: by the workgroup's first wave, for its seven siblings.  What a part decides - the
// box, the first empty pixel, the lights' ballot, whether it stands settled - is the same in every wave (every operand is), and in
// k_lighting_stand every wave works it out for itself: 88 vector and 67 scalar instructions ahead of the exit, in all 32 640 waves of a
// 1920 x 1080 launch of which two thirds then return - a third of the kernel's vector issue and two thirds of its scalar issue.  Here wave
// 0 takes the one trip (records, mark, the lane's light), decides, and leaves in LDS what the others need: the ballot, the first empty
// pixel, settled or not, and the eight waves' empty-pixel masks (lanes 48 - 63 store their record word as it came).  The others wait at
// a barrier and read it back: a wave of a settled part runs its slice of the next map's clear and returns behind two LDS reads.
//  - Values, comparisons and their order are k_lighting_stand's - rest_decide is the one copy of them -: every bit of every frame is.
//  - The mark has one reader now, wave 0, so thread 0 updates it right behind its own read: no sibling can see the store.
//  - A part that shades pays one barrier more than k_lighting_stand (the set-up's second is the tables').
template <bool BACKGROUND, int TB>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(ZR_LIGHT_KEPT_WAVES, ZR_LIGHT_KEPT_WAVES)))
void k_lighting_lead(ZrLightParams L, ZrRestArgs R, const uint32_t* __restrict__ owned_tiles, GBufferPtrs G, const float* __restrict__ srgb_lut,
                     const float* __restrict__ unorm_lut, uint32_t* __restrict__ out, const float4* __restrict__ plane, const float4* __restrict__ rest,
                     uint32_t* marks, uint32_t gen)
{
    static_assert(sizeof(ZrLightParams) + sizeof(ZrRestArgs) + sizeof(GBufferPtrs) + 8 * sizeof(void*) + 256 /* the hidden arguments */ < 4096,
                  "k_lighting_lead: the argument block");
    constexpr uint32_t PARTS = TILE_PIX / (uint32_t)TB, WAVES = (uint32_t)TB / 64u;
    static_assert(WAVES <= 8u && 1536u % (uint32_t)TB == 0u, "k_lighting_lead: a part's records are a dword per lane");
    __shared__ float tab[1536];          // rest_tables_load's
    __shared__ uint32_t empty_px;
    __shared__ uint32_t pub[20];         // wave 0's findings: [0], [1] the ballot, [2] the first empty pixel, [3] settled, [4 + w], [12 + w] the halves of wave w's mask
    const uint32_t part = blockIdx.x % PARTS, tile_slot = blockIdx.x / PARTS;
    const uint32_t i = threadIdx.x + part * (uint32_t)TB;      // the thread's pixel among the tile's
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave == 0u) {      // k_lighting_stand's trip and rest_decide, once
        const uint32_t rec = rest_records_fetch<WAVES>(rest, tile_slot * ZR_REST_RECORDS_PER_TILE + part * WAVES);
        const ZrRestLight* const lights = R.pt;
        const ArgLight mine_light{ &lights[lane < R.nPoint ? lane : 0u] };
        const uint32_t mark = (uint32_t)__builtin_amdgcn_readfirstlane((int)marks[blockIdx.x]);
        const RestDecision d = rest_decide<WAVES>(rec, mark, mine_light, R.nPoint, gen);
        if (lane >= 48u) pub[4u + (lane - 48u)] = (lane & 7u) < WAVES ? rec : 0u;
        if (lane == 0u) {
            pub[0] = (uint32_t)d.reach; pub[1] = (uint32_t)(d.reach >> 32); pub[2] = d.first; pub[3] = d.settled ? 1u : 0u;
            if (gen != 0u && !d.settled) {
                if (d.reach == 0ull) marks[blockIdx.x] = gen;            // (it did not stand)
                else if (mark == gen) marks[blockIdx.x] = 0u;
            }
        }
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane((int)pub[3]) != 0) { light_clear_next_slice<TB>(L); return; }
    const unsigned long long reach = (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)pub[0]) |
                                     (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)pub[1]) << 32;
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)pub[2]);      // (the same for every thread of the workgroup: wave 0's finding)
    const unsigned long long mine = (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)pub[4u + wave]) |
                                    (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)pub[12u + wave]) << 32;
    rest_tables_load<TB>(tab, srgb_lut, unorm_lut);
    const uint32_t tile = owned_tiles[tile_slot];
    __syncthreads();
    light_clear_next_slice<TB>(L);
    rest_shade_part<true, BACKGROUND>(L, R, G, tab, out, plane, rest, reach, first, mine, tile, tile_slot, i, &empty_px);
}
#endif

// GBufferVis (SH/BaseLighting.frag:42-145, SPEC_CONSTANTS 9).  Runs after k_lighting has written FinalColor everywhere: the
// lighting quad samples every GBuffer target again at UV = fragTexCoord * 3 / (1 - EmptyRatio) through LINEAR / REPEAT samplers
// (ZE:2811-2847) and shows a 3 x 3 mosaic; the centre cell and whatever lies outside the cells keep FinalColor.  Bilinear
// weights are snapped to 8 fractional bits (a stated choice, like sampling hardware): with EmptyRatio = 0 every sample is
// exactly texel (3x + 1, 3y + 1) mod (W, H).
struct GTexel { float v[20]; };     // SceneColor, GBufferA, B, C, D as five vec4
__device__ __forceinline__ GTexel gbuffer_texel(const GBufferPtrs& G, uint32_t W, int x, int y)
{
    const size_t p = (size_t)y * W + (size_t)x;
    const uint32_t sc = G.scene_color[p], A = G.gA[p], B = G.gB[p], C = G.gC[p];
    const uint2 D = G.gD[p];
    GTexel t;
    for (int k = 0; k < 4; ++k) {
        t.v[k] = (float)((sc >> (8 * k)) & 255u) / 255.0f;
        t.v[8 + k] = (float)((B >> (8 * k)) & 255u) / 255.0f;
        t.v[12 + k] = (float)((C >> (8 * k)) & 255u) / 255.0f;
    }
    t.v[4] = (float)((A >> 20) & 1023u) / 1023.0f; t.v[5] = (float)((A >> 10) & 1023u) / 1023.0f;
    t.v[6] = (float)(A & 1023u) / 1023.0f; t.v[7] = (float)(A >> 30) / 3.0f;
    t.v[16] = zr_f16_to_f32(D.x & 0xFFFFu); t.v[17] = zr_f16_to_f32(D.x >> 16);
    t.v[18] = zr_f16_to_f32(D.y & 0xFFFFu); t.v[19] = zr_f16_to_f32(D.y >> 16);
    return t;
}
__device__ __forceinline__ int wrap_index(int i, int n) { const int m = i % n; return m < 0 ? m + n : m; }

__global__ __launch_bounds__(256) void k_gbuffer_vis(ZrLightParams L, const XkView* __restrict__ view, GBufferPtrs G,
                                                     const float* __restrict__ shadowmap, CubeDesc C,
                                                     const float* __restrict__ srgb_lut, uint32_t* __restrict__ out)
{
    const uint32_t px = blockIdx.x * 16u + (threadIdx.x & 15u), py = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (px >= L.W || py >= L.H) return;
    const float ERx = view->ViewportInfo[2] / view->ViewportInfo[0], ERy = view->ViewportInfo[3] / view->ViewportInfo[1];
    const float tx = ((float)px + 0.5f) / (float)L.W, ty = ((float)py + 0.5f) / (float)L.H;        // fragTexCoord
    const float UVx = (tx * 3.0f) / (1.0f - ERx), UVy = (ty * 3.0f) / (1.0f - ERy);
    const float Sx = (1.0f - ERx) / 3.0f, Sy = (1.0f - ERy) / 3.0f;                                 // Step
    int cell = -1; float bx = 0.0f, by = 0.0f;
    if (tx < Sx && ty < Sy) { cell = 0; bx = 1.0f; by = 1.0f; }
    else if (tx < Sx * 2.0f && ty < Sy) { cell = 1; bx = 2.0f; by = 1.0f; }
    else if (tx < Sx * 3.0f && ty < Sy) { cell = 2; bx = 3.0f; by = 1.0f; }
    else if (tx < Sx && ty < Sy * 2.0f) { cell = 3; bx = 1.0f; by = 2.0f; }
    else if (tx < 1.0f && ty < Sy * 2.0f && tx > Sx * 2.0f) { cell = 4; bx = 3.0f; by = 2.0f; }
    else if (tx < Sx && ty < Sx * 3.0f) { cell = 5; bx = 1.0f; by = 3.0f; }                         // Step.x * 3: as the shader has it
    else if (tx < Sx * 2.0f && tx > Sx && ty < Sy * 3.0f && ty > Sy * 2.0f) { cell = 6; bx = 2.0f; by = 3.0f; }
    else if (tx < Sx * 3.0f && tx > Sx * 2.0f && ty < Sy * 3.0f && ty > Sy * 2.0f) { cell = 7; bx = 3.0f; by = 3.0f; }
    if (cell < 0) return;                                                                           // FinalColor stays
    zf3 o;
    if (tx > Sx * (bx - ERx) || ty > Sy * (by - ERy)) o = zr3(1.0f, 1.0f, 1.0f);                      // the cells' white frames
    else {
        // texture(sampler2D, UV): one mip level, LINEAR, REPEAT
        float x = __builtin_fmaf(UVx, (float)L.W, -0.5f), y = __builtin_fmaf(UVy, (float)L.H, -0.5f);
        if (!(__builtin_fabsf(x) < 1.0e9f)) x = 0.0f;
        if (!(__builtin_fabsf(y) < 1.0e9f)) y = 0.0f;
        const float fx = __builtin_floorf(x), fy = __builtin_floorf(y);
        const float ax = __builtin_floorf(__builtin_fmaf(x - fx, 256.0f, 0.5f)) / 256.0f;
        const float ay = __builtin_floorf(__builtin_fmaf(y - fy, 256.0f, 0.5f)) / 256.0f;
        const int x0 = wrap_index((int)fx, (int)L.W), x1 = wrap_index((int)fx + 1, (int)L.W);
        const int y0 = wrap_index((int)fy, (int)L.H), y1 = wrap_index((int)fy + 1, (int)L.H);
        const GTexel t00 = gbuffer_texel(G, L.W, x0, y0), t10 = gbuffer_texel(G, L.W, x1, y0);
        const GTexel t01 = gbuffer_texel(G, L.W, x0, y1), t11 = gbuffer_texel(G, L.W, x1, y1);
        float g[20];
        for (int k = 0; k < 20; ++k) {
            const float top = __builtin_fmaf(ax, t10.v[k] - t00.v[k], t00.v[k]), bot = __builtin_fmaf(ax, t11.v[k] - t01.v[k], t01.v[k]);
            g[k] = __builtin_fmaf(ay, bot - top, top);
        }
        const zf3 BaseColor = zr3(g[12], g[13], g[14]);
        const float Metallic = zr_saturate(g[8]);
        const float Roughness = __builtin_fmaxf(0.01f, zr_saturate(g[10]));
        const zf3 Normal = zr3(__builtin_fmaf(g[4], 2.0f, -1.0f), __builtin_fmaf(g[5], 2.0f, -1.0f), __builtin_fmaf(g[6], 2.0f, -1.0f));
        const float AO = zr_saturate(g[15]);
        const zf3 N = zr_normalize(Normal);
        const zf3 Pw = zr3(g[16], g[17], g[18]);
        switch (cell) {
        case 0: o = gamma3(BaseColor); break;
        case 1: o = zr3(Metallic, Metallic, Metallic); break;
        case 2: o = zr3(Roughness, Roughness, Roughness); break;
        case 3: o = N; break;
        case 4: o = zr3(AO, AO, AO); break;
        case 5: o = zr3(0.0f, 0.0f, 0.0f); break;
        case 6: {
            const zf3 cam = zr3(view->CameraInfo[0], view->CameraInfo[1], view->CameraInfo[2]);
            const zf3 Vv = zr_normalize(cam - Pw), Nn = zr_normalize(N);
            o = cube_sample(C, srgb_lut, L.cube_dim, (int)L.cube_levels, shade_refract(Nn, Vv), 0.0f) * 10.0f;
            break;
        }
        default: {
            const zf4 s4 = zr_mat4_point(L.SB, Pw);
            const float sx = s4.x / s4.w, sy = s4.y / s4.w, sz = s4.z / s4.w, sw = s4.w / s4.w;
            const float dxy = 1.5f * 1.0f / (float)L.SD;
            float sum = 0.0f;
            for (int xo = -2; xo <= 2; ++xo)
                for (int yo = -2; yo <= 2; ++yo) sum += shadow_tap(shadowmap, (int)L.SD, sx, sy, sz, sw, dxy * (float)xo, dxy * (float)yo);
            const float sf = sum * 0.04f;
            o = zr3(sf, sf, sf);
            break;
        }
        }
    }
    out[(size_t)py * L.W + px] = pack_rgb8(o);
}

// ------------------------------------------------------------------------------------------------ launchers (C++ linkage, used by zr_frame_host.cpp)

void zr_launch_lighting(const ZrLightParams& L, const XkView* view, const uint32_t* owned_tiles, uint32_t n_owned,
                        const GBufferPtrs& G, const float* shadowmap, const CubeDesc& C, const float* lut, const float* unorm_lut,
                        uint32_t* out, hipStream_t s, ZrLightMode mode, float4* plane, float4* rest)
{
    if (n_owned == 0) return;
    if (!plane) mode = ZR_LIGHT_PLAIN;      // (no plane: nothing to fill or to read)
    if (mode != ZR_LIGHT_FILL) rest = nullptr;
    // with several point lights each tile first builds its light list (L.light_list: decided on the host from the light count)
#define ZR_LAUNCH_LIGHTING_TB(LL, BG, TB, MODE) hipLaunchKernelGGL((k_lighting<LL, BG, TB, ZR_PIXELS_PER_THREAD, MODE>), dim3(n_owned * (TILE_PIX / ZR_PIXELS_PER_THREAD / TB)), dim3(TB), 0, s, L, view, owned_tiles, G, shadowmap, C, lut, unorm_lut, out, plane, rest)
#define ZR_LAUNCH_LIGHTING(LL, BG) do { if (mode == ZR_LIGHT_KEPT) ZR_LAUNCH_LIGHTING_TB(LL, BG, ZR_LIGHT_KEPT_TB, ZR_LIGHT_KEPT); \
                                        else if (mode == ZR_LIGHT_FILL) ZR_LAUNCH_LIGHTING_TB(LL, BG, ZR_LIGHT_TB, ZR_LIGHT_FILL); \
                                        else ZR_LAUNCH_LIGHTING_TB(LL, BG, ZR_LIGHT_TB, ZR_LIGHT_PLAIN); } while (0)
    if (L.light_list) { if (L.bg_enabled) ZR_LAUNCH_LIGHTING(true, true); else ZR_LAUNCH_LIGHTING(true, false); }
    else { if (L.bg_enabled) ZR_LAUNCH_LIGHTING(false, true); else ZR_LAUNCH_LIGHTING(false, false); }
#undef ZR_LAUNCH_LIGHTING
#undef ZR_LAUNCH_LIGHTING_TB
}
bool zr_lighting_rest_available() { return ZR_PIXELS_PER_THREAD == 1; }
// The resting frame's launch.  which: every pixel (k_lighting_rest), or the parts no point light reaches left as they stand, decided in
// every wave (k_lighting_stand) or once a part (k_lighting_lead): the same frame, the same marks.
// marks: a word per workgroup of the launch (n_owned * zr_lighting_stand_parts()); gen: zr_settle.h's generation, 0 = off
uint32_t zr_lighting_stand_parts() { return TILE_PIX / ZR_LIGHT_KEPT_TB; }
void zr_launch_lighting_rest(const ZrLightParams& L, const ZrRestArgs& R, const uint32_t* owned_tiles, uint32_t n_owned, const GBufferPtrs& G,
                             const float* lut, const float* unorm_lut, uint32_t* out, hipStream_t s, const float4* plane, const float4* rest,
                             ZrRestLaunch which, uint32_t* marks, uint32_t gen)
{
#if ZR_PIXELS_PER_THREAD == 1
    if (n_owned == 0) return;
    const dim3 grid(n_owned * (TILE_PIX / ZR_LIGHT_KEPT_TB)), block(ZR_LIGHT_KEPT_TB);
    constexpr int TB = ZR_LIGHT_KEPT_TB;
    const bool bg = L.bg_enabled;
    auto launch = [&](auto kernel, auto... more) { hipLaunchKernelGGL(kernel, grid, block, 0, s, L, R, owned_tiles, G, lut, unorm_lut, out, plane, rest, more...); };
    if (which == ZR_REST_LEAD) launch(bg ? k_lighting_lead<true, TB> : k_lighting_lead<false, TB>, marks, gen);
    else if (which == ZR_REST_STAND) launch(bg ? k_lighting_stand<true, TB> : k_lighting_stand<false, TB>, marks, gen);
    else if (L.light_list) launch(bg ? k_lighting_rest<true, true, TB> : k_lighting_rest<true, false, TB>);
    else launch(bg ? k_lighting_rest<false, true, TB> : k_lighting_rest<false, false, TB>);
#endif
}
void zr_launch_gbuffer_vis(const ZrLightParams& L, const XkView* view, const GBufferPtrs& G, const float* shadowmap, const CubeDesc& C,
                           const float* lut, uint32_t* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_gbuffer_vis, dim3((L.W + 15) / 16, (L.H + 15) / 16), dim3(256), 0, s, L, view, G, shadowmap, C, lut, out);
}
