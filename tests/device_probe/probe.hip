// probe.hip — TEST-ONLY: runs the product's device functions one call per thread, so a test can hold each of them to the CPU oracle over
// a table of operands (tests/test_gpu_device_functions.py).  It includes the product's headers and defines no arithmetic of its own: every
// kernel below loads a case's words, calls the function under test, and stores the result words.  The product never names this file.
//
// A case is IN[fn] 32-bit words in and OUT[fn] words out (floats as their bits); thread i handles case i, bounds-checked against n.
#include "../../zeldaengine_amd/csrc/zr_shade.h"
#include "../../zeldaengine_amd/csrc/zr_surface.h"
#include "../../zeldaengine_amd/csrc/zr_ctx.h"          // kSlotPack: where each material slot's channels sit in a packed texel

#include <cstring>

#define ZP_OK 0
#define ZP_ERR_ARG -1
#define ZP_ERR_HIP -2

enum {
    ZP_RSQRT = 0, ZP_SINCOS, ZP_EXP2, ZP_LOG2, ZP_POW, ZP_POW5, ZP_SATURATE, ZP_CLAMP, ZP_UNORM, ZP_F16_TO_F32, ZP_F32_TO_F16, ZP_UNORM8,
    ZP_DIV, ZP_SQRT, ZP_DOT, ZP_CROSS, ZP_NORMALIZE, ZP_TANGENT_NORMAL, ZP_MAT4_POINT,
    ZP_INSTANCE_RECORD, ZP_VS_POSITION, ZP_VS_NORMAL, ZP_CLASSIFY, ZP_PROJECT,
    ZP_F_SCHLICK, ZP_FR_DISNEY, ZP_V_SMITH, ZP_D_GGX, ZP_SHADOW_TAP,
    ZP_CUBE_SAMPLE, ZP_PCF_TAPS, ZP_SHADE, ZP_SHADE_MASKED,
    ZP_TEX_FOOTPRINT, ZP_TEX_IMAGE, ZP_TEX_MATERIAL, ZP_TEX_PACKED, ZP_BARY_SCREEN, ZP_BARY_HOMOG, ZP_INTERP, ZP_COMPUTE_NORMAL, ZP_MODEL_POINT,
    ZP_F32_TO_F16_HW, ZP_F16_TO_F32_HW, ZP_COUNT
};
//                                      rsq sc ex lg pw p5 sat cl un h2f f2h u8 div sq dot cr nrm tsn m4p  inst vsp vsn cls prj  Fs Fd Vs Dg tap cube pcf shade masked fp img mat pk  bs  bh  ip  cn  mp  f2h h2f
constexpr int zp_in(int fn)  { constexpr int t[ZP_COUNT] = { 1, 1, 1, 1, 2, 1, 1,  3, 2, 1,  1,  1, 2,  1, 6,  6, 3,  3,  19,  8,   19, 36, 12, 6,   3, 4, 3, 2, 6, 4, 3, 23, 23,   7, 6,  6,  6,  11, 16, 12, 16, 20, 1,  1 }; return t[fn]; }
constexpr int zp_out(int fn) { constexpr int t[ZP_COUNT] = { 1, 2, 1, 1, 1, 1, 1,  1, 1, 1,  1,  1, 1,  1, 1,  3, 3,  3,  4,   16,  3,  3,  1,  4,   1, 1, 1, 1, 1, 3, 1, 10, 10,   4, 4,  28, 13, 3,  3,  4,  3,  3,  1,  1 }; return t[fn]; }

// What the functions that read more than their case are handed (device pointers): the shadow map, the cubemap's mip chain and its sRGB
// decode table, the frame's XkView, and the lighting pass's uniforms as k_lighting holds them; for the sampler a draw record whose material
// slots (and packed form) hold the run's images, and which slot tex_image samples, as sRGB or UNORM.
struct ZpDev {
    const float* map; int SD;
    CubeDesc cube; const float* lut;
    const XkView* view; ZrLightParams L;
    uint32_t nDir, nPoint; float maxmips, dxy;
    const ZrObject* obj; int slot, srgb;
};

__device__ __forceinline__ void put3(uint32_t* o, zf3 v) { o[0] = zr_f2u(v.x); o[1] = zr_f2u(v.y); o[2] = zr_f2u(v.z); }

template <int FN>
__global__ void k_probe(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, const ZpDev D)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* a = in + (size_t)i * zp_in(FN);
    uint32_t* o = out + (size_t)i * zp_out(FN);
    float f[36];
#pragma unroll
    for (int k = 0; k < zp_in(FN); ++k) f[k] = zr_u2f(a[k]);
    if constexpr (FN == ZP_RSQRT) o[0] = zr_f2u(zr_rsqrt(f[0]));
    else if constexpr (FN == ZP_SINCOS) { float s, c; zr_sincos(f[0], s, c); o[0] = zr_f2u(s); o[1] = zr_f2u(c); }
    else if constexpr (FN == ZP_EXP2) o[0] = zr_f2u(zr_exp2(f[0]));
    else if constexpr (FN == ZP_LOG2) o[0] = zr_f2u(zr_log2(f[0]));
    else if constexpr (FN == ZP_POW) o[0] = zr_f2u(zr_pow(f[0], f[1]));
    else if constexpr (FN == ZP_POW5) o[0] = zr_f2u(zr_pow5(f[0]));
    else if constexpr (FN == ZP_SATURATE) o[0] = zr_f2u(zr_saturate(f[0]));
    else if constexpr (FN == ZP_CLAMP) o[0] = zr_f2u(zr_clamp(f[0], f[1], f[2]));
    else if constexpr (FN == ZP_UNORM) o[0] = zr_unorm(f[0], f[1]);
    else if constexpr (FN == ZP_F16_TO_F32) o[0] = zr_f2u(zr_f16_to_f32(a[0]));
    else if constexpr (FN == ZP_F32_TO_F16) o[0] = zr_f32_to_f16(f[0]);
    else if constexpr (FN == ZP_UNORM8) { const float c = (float)(a[0] & 255u); o[0] = zr_f2u(__builtin_fmaf(c, ZR_UNORM8_HI, c * ZR_UNORM8_LO)); }
    else if constexpr (FN == ZP_DIV) o[0] = zr_f2u(f[0] / f[1]);
    else if constexpr (FN == ZP_SQRT) o[0] = zr_f2u(__builtin_sqrtf(f[0]));
    else if constexpr (FN == ZP_DOT) o[0] = zr_f2u(zr_dot(zr3(f[0], f[1], f[2]), zr3(f[3], f[4], f[5])));
    else if constexpr (FN == ZP_CROSS) put3(o, zr_cross(zr3(f[0], f[1], f[2]), zr3(f[3], f[4], f[5])));
    else if constexpr (FN == ZP_NORMALIZE) put3(o, zr_normalize(zr3(f[0], f[1], f[2])));
    else if constexpr (FN == ZP_TANGENT_NORMAL) put3(o, zr_tangent_space_normal(zr3(f[0], f[1], f[2])));
    else if constexpr (FN == ZP_MAT4_POINT) {
        const zf4 r = zr_mat4_point(f, zr3(f[16], f[17], f[18]));
        o[0] = zr_f2u(r.x); o[1] = zr_f2u(r.y); o[2] = zr_f2u(r.z); o[3] = zr_f2u(r.w);
    } else if constexpr (FN == ZP_INSTANCE_RECORD) {
        XkInstanceData d;
        __builtin_memcpy(&d, f, sizeof d);
        const ZrInstance I = instance_record(d);
        static_assert(sizeof(XkInstanceData) == 32 && sizeof(ZrInstance) == 64, "case layout");
        const uint32_t* w = (const uint32_t*)&I;
#pragma unroll
        for (int k = 0; k < 16; ++k) o[k] = w[k];
    } else if constexpr (FN == ZP_VS_POSITION) {        // p, then a ZrInstance
        ZrInstance I;
        __builtin_memcpy(&I, f + 3, sizeof I);
        put3(o, vs_position(zr3(f[0], f[1], f[2]), I, true));
    } else if constexpr (FN == ZP_VS_NORMAL) {          // n, a ZrInstance, M, instanced
        ZrInstance I;
        __builtin_memcpy(&I, f + 3, sizeof I);
        put3(o, vs_normal(zr3(f[0], f[1], f[2]), I, a[35] != 0u, f + 19));
    } else if constexpr (FN == ZP_CLASSIFY) {           // three clip-space corners
        zf4 c[3];
        __builtin_memcpy(c, f, sizeof c);
        o[0] = (uint32_t)classify(vertex_flags(c[0]), vertex_flags(c[1]), vertex_flags(c[2]));
    } else if constexpr (FN == ZP_PROJECT) {            // a clip-space corner, half width, half height
        zf4 c;
        __builtin_memcpy(&c, f, sizeof c);
        const SV s = project(c, f[4], f[5]);
        o[0] = (uint32_t)s.X; o[1] = (uint32_t)s.Y; o[2] = zr_f2u(s.z); o[3] = zr_f2u(s.rw);
    } else if constexpr (FN == ZP_F_SCHLICK) o[0] = zr_f2u(F_Schlick(f[0], f[1], f[2]));
    else if constexpr (FN == ZP_FR_DISNEY) o[0] = zr_f2u(Fr_DisneyDiffuse(f[0], f[1], f[2], f[3]));
    else if constexpr (FN == ZP_V_SMITH) o[0] = zr_f2u(V_SmithGGXCorrelated(f[0], f[1], f[2]));
    else if constexpr (FN == ZP_D_GGX) o[0] = zr_f2u(D_GGX(f[0], f[1]));
    else if constexpr (FN == ZP_SHADOW_TAP) o[0] = zr_f2u(shadow_tap(D.map, D.SD, f[0], f[1], f[2], f[3], f[4], f[5]));
    else if constexpr (FN == ZP_CUBE_SAMPLE) put3(o, cube_sample(D.cube, D.lut, D.L.cube_dim, (int)D.L.cube_levels, zr3(f[0], f[1], f[2]), f[3]));
    else if constexpr (FN == ZP_PCF_TAPS) {             // ComputePCF as 25 calls of shadow_tap in the shader's order: the per-texel statement of the PCF block
        const zf4 s4 = zr_mat4_point(D.L.SB, zr3(f[0], f[1], f[2]));
        const float sx = s4.x / s4.w, sy = s4.y / s4.w, sz = s4.z / s4.w, sw = s4.w / s4.w;
        float sum = 0.0f;
        for (int x = -2; x <= 2; ++x)
            for (int y = -2; y <= 2; ++y) sum += shadow_tap(D.map, D.SD, sx, sy, sz, sw, D.dxy * (float)x, D.dxy * (float)y);
        o[0] = zr_f2u(sum * 0.04f);
    } else if constexpr (FN == ZP_SHADE || FN == ZP_SHADE_MASKED) {
        // cam, BaseColor, Metallic, Roughness, N, AO, P, then 8 words of point-light mask (read by the masked form only)
        zf3 Direct, Indirect, RefC; float SF;
        shade_surface<FN == ZP_SHADE_MASKED>(D.L, D.view, D.map, D.cube, D.lut, a + 15, D.nDir, D.nPoint, D.maxmips, D.dxy, zr3(f[0], f[1], f[2]),
                                             zr3(f[3], f[4], f[5]), f[6], f[7], zr3(f[8], f[9], f[10]), f[11], zr3(f[12], f[13], f[14]),
                                             Direct, Indirect, RefC, SF);
        put3(o, Direct); put3(o + 3, Indirect); put3(o + 6, RefC); o[9] = zr_f2u(SF);
    } else if constexpr (FN == ZP_TEX_FOOTPRINT) {      // w, h, levels of an image (no texel is read), then dudx, dvdx, dudy, dvdy
        ZrTex T;
        T.data = nullptr; T.w = a[0]; T.h = a[1]; T.levels = a[2]; T._pad = 0u;
        const TexFootprint F = tex_footprint(T, f[3], f[4], f[5], f[6]);
        o[0] = (uint32_t)F.N; o[1] = zr_f2u(F.lambda); o[2] = zr_f2u(F.du); o[3] = zr_f2u(F.dv);
    } else if constexpr (FN == ZP_TEX_IMAGE) {          // u, v, dudx, dvdx, dudy, dvdy; a slot without an image takes the constant arm
        const zf4 r = tex_sample<1>(D.obj->tex[D.slot], D.obj->texc[D.slot], D.srgb != 0, D.lut, f[0], f[1], f[2], f[3], f[4], f[5]);
        o[0] = zr_f2u(r.x); o[1] = zr_f2u(r.y); o[2] = zr_f2u(r.z); o[3] = zr_f2u(r.w);
    } else if constexpr (FN == ZP_TEX_MATERIAL) {
        zf4 ms[ZR_MATERIAL_SLOTS];
        tex_sample_material(D.obj, D.lut, f[0], f[1], f[2], f[3], f[4], f[5], ms);
#pragma unroll
        for (int s = 0; s < ZR_MATERIAL_SLOTS; ++s) { o[4 * s] = zr_f2u(ms[s].x); o[4 * s + 1] = zr_f2u(ms[s].y); o[4 * s + 2] = zr_f2u(ms[s].z); o[4 * s + 3] = zr_f2u(ms[s].w); }
    } else if constexpr (FN == ZP_TEX_PACKED) {
        float pk[ZR_PK_CHANNELS];
        tex_sample_packed(D.obj->packed, D.lut, f[0], f[1], f[2], f[3], f[4], f[5], pk);
#pragma unroll
        for (int k = 0; k < ZR_PK_CHANNELS; ++k) o[k] = zr_f2u(pk[k]);
    } else if constexpr (FN == ZP_BARY_SCREEN) {        // a FastSetup as pixel_geom fills it, px, py
        FastSetup fs;
        fs.X0 = (int)a[0]; fs.Y0 = (int)a[1]; fs.a1 = f[2]; fs.b1 = f[3]; fs.a2 = f[4]; fs.b2 = f[5]; fs.rw0 = f[6]; fs.rw1 = f[7]; fs.rw2 = f[8];
        const Bary b = bary_screen(fs, (int)a[9], (int)a[10]);
        o[0] = zr_f2u(b.b0); o[1] = zr_f2u(b.b1); o[2] = zr_f2u(b.b2);
    } else if constexpr (FN == ZP_BARY_HOMOG) {         // three clip-space corners, hw, hh, px, py
        zf4 c[3];
        __builtin_memcpy(c, f, sizeof c);
        const Bary b = bary_homog(c, f[12], f[13], (int)a[14], (int)a[15]);
        o[0] = zr_f2u(b.b0); o[1] = zr_f2u(b.b1); o[2] = zr_f2u(b.b2);
    } else if constexpr (FN == ZP_INTERP) {             // b, three vec3 attributes: interp3 of them, interp1 of (A0.x, A1.y, A2.z)
        Bary b; b.b0 = f[0]; b.b1 = f[1]; b.b2 = f[2];
        put3(o, interp3(b, zr3(f[3], f[4], f[5]), zr3(f[6], f[7], f[8]), zr3(f[9], f[10], f[11])));
        o[3] = zr_f2u(interp1(b, f[3], f[7], f[11]));
    } else if constexpr (FN == ZP_COMPUTE_NORMAL) {     // pos_dx, pos_dy, s1, t1, s2, t2, fragN, ts
        put3(o, compute_normal(zr3(f[0], f[1], f[2]), zr3(f[3], f[4], f[5]), f[6], f[7], f[8], f[9], zr3(f[10], f[11], f[12]), zr3(f[13], f[14], f[15])));
    } else if constexpr (FN == ZP_MODEL_POINT) {        // M, p, m_identity
        ZrPass P;
        __builtin_memcpy(P.M, f, sizeof P.M);
        P.m_identity = a[19];
        put3(o, model_point(P, zr3(f[16], f[17], f[18])));
    } else if constexpr (FN == ZP_F32_TO_F16_HW) o[0] = f32_to_f16_hw(f[0]);
    else if constexpr (FN == ZP_F16_TO_F32_HW) o[0] = zr_f2u(f16_to_f32_hw(a[0]));
}

namespace {
struct DevBuf {           // frees on every way out of zp_run
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

template <int FN>
hipError_t launch(const uint32_t* in, uint32_t* out, uint32_t n, const ZpDev& D)
{
    hipLaunchKernelGGL(k_probe<FN>, dim3((n + 255u) / 256u), dim3(256), 0, 0, in, out, n, D);
    return hipGetLastError();
}
template <int FN>
hipError_t dispatch(int fn, const uint32_t* in, uint32_t* out, uint32_t n, const ZpDev& D)
{
    if constexpr (FN >= ZP_COUNT) return hipErrorInvalidValue;
    else return fn == FN ? launch<FN>(in, out, n, D) : dispatch<FN + 1>(fn, in, out, n, D);
}
hipError_t upload(DevBuf& b, const void* host, size_t bytes)
{
    hipError_t e = hipMalloc(&b.p, bytes);
    return e == hipSuccess ? hipMemcpy(b.p, host, bytes, hipMemcpyHostToDevice) : e;
}
}

// Host-side description of what a case's function reads besides the case (any part may be absent; a function that needs it then fails
// with ZP_ERR_ARG): a square shadow map; a cubemap as its whole mip chain, level after level (level l: 6 faces of (dim >> l)^2 RGBA8
// texels, floor(log2 dim) + 1 levels) with the 256-entry decode table; an XkView; BiasMat * shadowmapSpace.
struct zp_scene {
    const float* map; int32_t map_dim;
    const uint8_t* cube; uint32_t cube_dim; const float* lut;
    const XkView* view;
    float SB[16];
};

extern "C" int zp_count(void) { return ZP_COUNT; }
extern "C" int zp_words_in(int fn) { return fn >= 0 && fn < ZP_COUNT ? zp_in(fn) : ZP_ERR_ARG; }
extern "C" int zp_words_out(int fn) { return fn >= 0 && fn < ZP_COUNT ? zp_out(fn) : ZP_ERR_ARG; }

// Runs function fn over n cases: allocate, copy in, launch, synchronise, copy out, free.  Returns ZP_OK, ZP_ERR_ARG, or ZP_ERR_HIP with the
// HIP error's number in *hip_error.
extern "C" int zp_run_scene(int fn, const void* in, void* out, uint32_t n, const zp_scene* sc, int* hip_error)
{
    if (hip_error) *hip_error = 0;
    if (fn < 0 || fn >= ZP_COUNT || !in || !out || n == 0u || n > (1u << 22)) return ZP_ERR_ARG;
    if (fn == ZP_TEX_IMAGE || fn == ZP_TEX_MATERIAL || fn == ZP_TEX_PACKED) return ZP_ERR_ARG;           // zp_run_textures
    const bool shade = fn == ZP_SHADE || fn == ZP_SHADE_MASKED;
    const bool need_map = fn == ZP_SHADOW_TAP || fn == ZP_PCF_TAPS || shade, need_cube = fn == ZP_CUBE_SAMPLE || shade;
    if ((need_map || need_cube) && !sc) return ZP_ERR_ARG;
    if (need_map && (!sc->map || sc->map_dim < 8 || sc->map_dim > 4096)) return ZP_ERR_ARG;      // the PCF's 16-byte loads span 8 texels
    if (need_cube && (!sc->cube || !sc->lut || sc->cube_dim < 1u || sc->cube_dim > 1024u)) return ZP_ERR_ARG;
    if (shade && !sc->view) return ZP_ERR_ARG;
    ZpDev D;
    memset(&D, 0, sizeof D);
    const size_t bin = (size_t)n * zp_in(fn) * 4, bout = (size_t)n * zp_out(fn) * 4;
    DevBuf din, dout, dmap, dcube, dlut, dview;
    hipError_t e = upload(din, in, bin);
    if (e == hipSuccess) e = hipMalloc(&dout.p, bout);
    if (e == hipSuccess) e = hipMemset(dout.p, 0xCD, bout);
    if (e == hipSuccess && need_map) {
        e = upload(dmap, sc->map, (size_t)sc->map_dim * sc->map_dim * 4);
        D.map = (const float*)dmap.p; D.SD = sc->map_dim; D.L.SD = (uint32_t)sc->map_dim;
        D.dxy = 1.5f * 1.0f / (float)D.L.SD;                    // as k_lighting forms it
        memcpy(D.L.SB, sc->SB, sizeof D.L.SB);
    }
    if (e == hipSuccess && need_cube) {
        size_t off[16], total = 0;
        uint32_t levels = 0;
        for (uint32_t d = sc->cube_dim; ; d >>= 1) { off[levels++] = total; total += (size_t)d * d * 4 * 6; if (d <= 1u) break; }
        e = upload(dcube, sc->cube, total);
        if (e == hipSuccess) e = upload(dlut, sc->lut, 256 * 4);
        for (uint32_t l = 0; l < levels; ++l) D.cube.levels[l] = (const uint8_t*)dcube.p + off[l];
        D.lut = (const float*)dlut.p; D.L.cube_dim = sc->cube_dim; D.L.cube_levels = levels;
    }
    if (e == hipSuccess && shade) {
        const int nd = sc->view->LightsCount[0], np = sc->view->LightsCount[1];
        if (nd < 0 || nd > XK_MAX_DIRECTIONAL_LIGHTS_NUM || np < 0 || np > XK_MAX_POINT_LIGHTS_NUM || np > 256) return ZP_ERR_ARG;   // 8 mask words per case
        e = upload(dview, sc->view, sizeof(XkView));
        D.view = (const XkView*)dview.p; D.nDir = (uint32_t)nd; D.nPoint = (uint32_t)np;
        D.maxmips = (float)(uint32_t)sc->view->LightsCount[3];
    }
    if (e == hipSuccess) e = dispatch<0>(fn, (const uint32_t*)din.p, (uint32_t*)dout.p, n, D);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, bout, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        if (hip_error) *hip_error = (int)e;
        return ZP_ERR_HIP;
    }
    return ZP_OK;
}
extern "C" int zp_run(int fn, const void* in, void* out, uint32_t n) { return zp_run_scene(fn, in, out, n, nullptr, nullptr); }

// ---- the sampler (zr_texture.h): its images travel beside the table, as a material's seven slots.
// A slot is an image - its whole mip chain as the product holds it, level after level, `bytes` long - or, chain == nullptr, the constant
// `constant` (what the host decodes once into ZrObject::texc).  tex_image samples slot `image_slot` as sRGB (srgb != 0) or UNORM;
// tex_material samples all seven; tex_packed samples the packed form, which this function lays out from the chains by the product's
// kSlotPack, as zr_object_remake_material does.  What the product's host refuses is refused here (ZP_ERR_ARG): a side of 0 or above
// 16384, a level count that is not the chain's, more than 16 levels, and a packed form over images of different sizes - so no table can
// hand the kernels an image the product could not hold.
struct zp_slot { const uint8_t* chain; uint64_t bytes; uint32_t w, h, levels, texel; float constant[4]; };
struct zp_textures { zp_slot slot[ZR_MATERIAL_SLOTS]; const float* lut; int32_t image_slot, srgb; };

static bool chain_ok(const zp_slot& s)
{
    if (s.w == 0u || s.h == 0u || s.w > 16384u || s.h > 16384u || s.levels == 0u || s.levels > 16u) return false;
    uint32_t m = s.w > s.h ? s.w : s.h, levels = 1;
    while (m > 1u) { m >>= 1; ++levels; }
    uint64_t bytes = 0;
    for (uint32_t l = 0; l < levels; ++l) { uint32_t lw = s.w >> l, lh = s.h >> l; if (!lw) lw = 1; if (!lh) lh = 1; bytes += (uint64_t)lw * lh * 4u; }
    return levels == s.levels && bytes == s.bytes;
}

extern "C" int zp_run_textures(int fn, const void* in, void* out, uint32_t n, const zp_textures* tx, int* hip_error)
{
    if (hip_error) *hip_error = 0;
    if ((fn != ZP_TEX_IMAGE && fn != ZP_TEX_MATERIAL && fn != ZP_TEX_PACKED) || !in || !out || !tx || !tx->lut || n == 0u || n > (1u << 22)) return ZP_ERR_ARG;
    if (fn == ZP_TEX_IMAGE && (tx->image_slot < 0 || tx->image_slot >= ZR_MATERIAL_SLOTS)) return ZP_ERR_ARG;
    int lead = -1;
    for (int s = 0; s < ZR_MATERIAL_SLOTS; ++s) {
        const zp_slot& sl = tx->slot[s];
        if (!sl.chain) continue;
        if (!chain_ok(sl)) return ZP_ERR_ARG;
        if (lead < 0) lead = s;
        else if (fn == ZP_TEX_PACKED && (sl.w != tx->slot[lead].w || sl.h != tx->slot[lead].h)) return ZP_ERR_ARG;
    }
    if (fn == ZP_TEX_PACKED && lead < 0) return ZP_ERR_ARG;
    ZrObject O;
    memset(&O, 0, sizeof O);
    ZpDev D;
    memset(&D, 0, sizeof D);
    const size_t bin = (size_t)n * zp_in(fn) * 4, bout = (size_t)n * zp_out(fn) * 4;
    DevBuf din, dout, dlut, dobj, dpk, dtex[ZR_MATERIAL_SLOTS];
    hipError_t e = upload(din, in, bin);
    if (e == hipSuccess) e = hipMalloc(&dout.p, bout);
    if (e == hipSuccess) e = hipMemset(dout.p, 0xCD, bout);
    if (e == hipSuccess) e = upload(dlut, tx->lut, 256 * 4);
    for (int s = 0; s < ZR_MATERIAL_SLOTS && e == hipSuccess; ++s) {
        const zp_slot& sl = tx->slot[s];
        memcpy(O.texc[s], sl.constant, sizeof sl.constant);
        O.texel[s] = sl.texel;
        if (!sl.chain) { O.const_slots |= 1u << s; continue; }
        e = upload(dtex[s], sl.chain, (size_t)sl.bytes);
        O.tex[s].data = (const uint8_t*)dtex[s].p; O.tex[s].w = sl.w; O.tex[s].h = sl.h; O.tex[s].levels = sl.levels;
    }
    if (e == hipSuccess && fn == ZP_TEX_PACKED) {
        const size_t n_texels = (size_t)tx->slot[lead].bytes / 4;
        std::vector<uint8_t> pk(n_texels * 16, 0);
        for (int s = 0; s < ZR_MATERIAL_SLOTS; ++s) {
            const auto& k = kSlotPack[s];
            const uint8_t* src = tx->slot[s].chain;
            for (size_t i = 0; i < n_texels; ++i)
                for (uint32_t ch = 0; ch < k.n; ++ch) pk[i * 16 + k.ch + ch] = src ? src[i * 4 + ch] : (uint8_t)(tx->slot[s].texel >> (8 * ch));
        }
        e = upload(dpk, pk.data(), pk.size());
        O.packed.data = (const uint8_t*)dpk.p; O.packed.w = tx->slot[lead].w; O.packed.h = tx->slot[lead].h; O.packed.levels = tx->slot[lead].levels;
    }
    if (e == hipSuccess) e = upload(dobj, &O, sizeof O);
    D.obj = (const ZrObject*)dobj.p; D.lut = (const float*)dlut.p; D.slot = tx->image_slot; D.srgb = tx->srgb;
    if (e == hipSuccess) e = dispatch<0>(fn, (const uint32_t*)din.p, (uint32_t*)dout.p, n, D);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, bout, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        if (hip_error) *hip_error = (int)e;
        return ZP_ERR_HIP;
    }
    return ZP_OK;
}
// where slot `slot`'s channels sit in tex_packed's 13 result words (the product's kSlotPack): first channel and count
extern "C" int zp_slot_pack(int slot, uint32_t* first, uint32_t* count)
{
    if (slot < 0 || slot >= ZR_MATERIAL_SLOTS || !first || !count) return ZP_ERR_ARG;
    *first = kSlotPack[slot].ch; *count = kSlotPack[slot].n;
    return ZP_OK;
}
