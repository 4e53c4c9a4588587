// zr_dev.h — common ground of the kernel files (csrc/zr_*.hip): tile / wave constants, address-space-qualified loads, the vertex stage
// (Base.vert / BaseInstanced.vert / Shadowmap*.vert), wave reductions on the DPP network, the Hi-Z tests, the per-pixel kernels' grid shape.
//
// The render path is one .hip per pass; each compiles alone (-fno-gpu-rdc), what they share is header-only and inlined:
//   zr_cull.hip      k_instance_prep, k_cull_instances<MODE>, k_cull_box<MODE, WORKLIST>
//   zr_shadow.hip    shadow pass, meshlet-level binning: k_bin_count / k_scan / k_bin_fill, k_raster_chunks<LATE>, k_shadow_slow,
//                    k_shadow_occlusion<WORKLIST>, k_count_shadow
//   zr_camera.hip    camera pass, triangle-level binning: k_hiz_build, k_select, k_geom<HIZ, COUNT>, k_plan, k_tile<LAST>, k_sky_tiles
//   zr_resolve.hip   k_resolve_gbuffer: BaseScene.frag per pixel from the key buffer into the SoA GBuffer planes
//                    k_mark: the visibility history alone, for a frame whose resolve runs on the host's stream
//   zr_lighting.hip  k_lighting (BaseLighting.frag), k_gbuffer_vis (debug view 9)
//   zr_forward.hip   k_forward: the forward variant, Base.frag
//   zr_frame.hip     k_frame_begin, fills, k_untile / k_pack_tiles (multi-GPU composite)
//   zr_delta.hip     k_delta_mark, k_delta_pack: the frame as the tiles that differ from the last delivery
//   zr_raster.h      the rasteriser proper (raster_sub, the clipper) and the steps of the kernels that own a tile's keys (tile context,
//                    queued / recorded triangle, keys' clear and merge, slow-triangle record, unit claim): shadow and camera pass
//   zr_dev.h (this)  also the steps the cull, select and bin kernels and the rasterising waves share: the tile rectangle (TileRect), a work
//                    item's self-contained record (bin_entry), the LDS histogram over a rect's tiles, the meshlet head (meshlet_head)
//   zr_texture.h     texture(sampler2D): mips, trilinear, anisotropic; zr_surface.h: interpolation, ComputeNormal, BaseScene.frag's body
//   zr_shade.h       Common.glsl's BxDF, PCF, cubemap sampling and the body BaseLighting.frag and Base.frag share
//
// Replaces: SH/Shadowmap*.vert, SH/Base*.vert, SH/BaseScene.frag, SH/Background.vert + SH/BaseLighting.frag, SH/Base.frag,
// the fixed-function rasteriser/ROP state of RHICreateGraphicsPipelines (ZE:5094-5201) and the draw loops of
// RecordCommandBuffer (ZE:3239-3540).  Raster rules: DESIGN.md §4.
#pragma once
#include "zr_math.h"
#include "zr_types.h"

#include <algorithm>
#include <cstddef>

#define WAVE 64
#define TILE ZR_TILE
#define TILE_PIX (TILE * TILE)
// Shadow pass: a workgroup rasterises into a WINDOW = its tile plus an apron of ZR_SHADOW_APRON texels to the right and below, and a
// meshlet is listed only for the tiles that its box WITHOUT its last APRON columns / rows touches: every texel of the box still lies in
// the window of a listed tile, and a meshlet up to APRON + 1 texels across (the usual caster under a 1024^2 map: 9 texels) is listed ONCE
// where the plain tile grid listed it 1.64 times - and transformed and tested it as often.  The pass's depth test is a min, so texels that
// two windows both draw come out the same; the windows' keys are merged into the map with atomicMin as before.
// (A/B on the whole frame: apron 0 / 4 / 8 / 12 / 16 / 32 -> 5 030 / 5 060 / 5 165 / 5 187 / 4 995 / 4 830 Mpixel/s with 179 950 / - / 126 105 /
// - / 111 000 / 110 000 list entries for 110 000 meshlets: 12 is the widest window whose keys leave room for six workgroups per CU.)
#ifndef ZR_SHADOW_APRON
#define ZR_SHADOW_APRON 12
#endif
#define SPAN(MODE) ((MODE) == ZR_MODE_SHADOW ? TILE + ZR_SHADOW_APRON : TILE)       // edge of the key window of a rasteriser workgroup
#define SPAN_PIX(MODE) (SPAN(MODE) * SPAN(MODE))
#define QCAP 128u
#define RW (ZR_TILE >= 64 ? 8 : 4)          // waves per rasteriser workgroup: one 64x64 tile's keys (32 KB) are shared by 8 waves
#define RTHREADS (RW * WAVE)
#ifndef ZR_RASTER_WAVES_DEFER
#define ZR_RASTER_WAVES_DEFER 6              // waves per SIMD the shadow rasteriser is compiled for (the clipper is not in its loop: k_shadow_slow)
#endif
// Diagnostic work-skipping switches (attribution of kernel time) exist only in -DZR_DIAG builds: the product library has none.
#ifdef ZR_DIAG
#define ZR_DIAG_SKIP(x) (x)
#else
#define ZR_DIAG_SKIP(x) 0u
#endif

// ------------------------------------------------------------------------------------------------ helpers

struct SV { int X, Y; float z, rw; };          // snapped screen vertex (1/256 px), NDC depth, 1/w

__device__ __forceinline__ uint32_t wave_uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// Ordering point between LDS accesses of ONE wave (a lane reads what another lane of the same wave wrote).  The LDS
// executes a wave's DS instructions in issue order, so no s_waitcnt is needed: only the compiler must not reorder.
__device__ __forceinline__ void lds_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

__device__ __forceinline__ int find_object_work(const ZrObject* __restrict__ objs, int n, uint32_t w)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) { int mid = (lo + hi + 1) >> 1; if (objs[mid].work_base <= w) lo = mid; else hi = mid - 1; }
    return lo;
}
__device__ __forceinline__ int find_object_prim(const ZrObject* __restrict__ objs, int n, uint32_t p)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) { int mid = (lo + hi + 1) >> 1; if (objs[mid].prim_base <= p) lo = mid; else hi = mid - 1; }
    return lo;
}

// Loads through pointers that were themselves read from memory (ZrObject's fields, a bin record's three addresses).  The compiler cannot
// know what such a pointer points into and emits FLAT loads for it: those count on BOTH wait counters (every LDS access then waits for
// them and they for it), keep their 64-bit addresses in vector registers and can never be scalar.  All of these point into device memory
// that no kernel of the frame writes while it is read - scene data, or records an earlier kernel laid down - so the loads are spelled in
// the global address space (an SGPR base + a 32-bit lane offset) or, for a record every lane reads, in the constant one (scalar loads).
#define ZR_AS_GLOBAL __attribute__((address_space(1)))
#define ZR_AS_CONST __attribute__((address_space(4)))
typedef float zr_f4v __attribute__((ext_vector_type(4)));
typedef uint32_t zr_u2v __attribute__((ext_vector_type(2)));
typedef uint32_t zr_u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_global(const float4* p) { const zr_f4v v = *(const ZR_AS_GLOBAL zr_f4v*)p; return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ uint2 ld_global(const uint2* p) { const zr_u2v v = *(const ZR_AS_GLOBAL zr_u2v*)p; return make_uint2(v.x, v.y); }
__device__ __forceinline__ uint4 ld_global(const uint4* p) { const zr_u4v v = *(const ZR_AS_GLOBAL zr_u4v*)p; return make_uint4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ uint32_t ld_global(const uint32_t* p) { return *(const ZR_AS_GLOBAL uint32_t*)p; }
__device__ __forceinline__ float ld_global(const float* p) { return *(const ZR_AS_GLOBAL float*)p; }
__device__ __forceinline__ uint8_t ld_global(const uint8_t* p) { return *(const ZR_AS_GLOBAL uint8_t*)p; }
// a whole record (dwords): scalar loads when the address is wave-uniform, vector loads when it is not
template <class T> __device__ __forceinline__ T ld_record(const T* p)
{
    static_assert(sizeof(T) % 4 == 0, "dwords");
    T v;
    uint32_t* d = (uint32_t*)&v;
    const ZR_AS_CONST uint32_t* q = (const ZR_AS_CONST uint32_t*)p;
#pragma unroll
    for (uint32_t i = 0; i < sizeof(T) / 4; ++i) d[i] = q[i];
    return v;
}

// The instance record of one XkInstanceData (k_instance_prep at zr_object_add, k_instance_apply after an update: one arithmetic, so an
// updated record is bit-identical to the one zr_object_add makes from the same data).
// MakeRotMatrix (SH/Common.glsl:60-87): rotMat = mz * my * mx; mx(R.x) turns about Y, my(R.y) about Z, mz(R.z) about X
__device__ __forceinline__ ZrInstance instance_record(const XkInstanceData& d)
{
    ZrInstance I;
    float s, c, mx[9], my[9], mz[9], t[9];
    zr_sincos(d.InstanceRotation[0], s, c);
    mx[0] = c; mx[1] = 0; mx[2] = s;  mx[3] = 0; mx[4] = 1; mx[5] = 0;  mx[6] = -s; mx[7] = 0; mx[8] = c;
    zr_sincos(d.InstanceRotation[1], s, c);
    my[0] = c; my[1] = s; my[2] = 0;  my[3] = -s; my[4] = c; my[5] = 0;  my[6] = 0; my[7] = 0; my[8] = 1;
    zr_sincos(d.InstanceRotation[2], s, c);
    mz[0] = 1; mz[1] = 0; mz[2] = 0;  mz[3] = 0; mz[4] = c; mz[5] = s;  mz[6] = 0; mz[7] = -s; mz[8] = c;
    zr_mat3_mul(mz, my, t);
    zr_mat3_mul(t, mx, I.R);
    I.t[0] = d.InstancePosition[0]; I.t[1] = d.InstancePosition[1]; I.t[2] = d.InstancePosition[2];
    I.s = d.InstancePScale;
    I._pad[0] = I._pad[1] = I._pad[2] = 0.0f;
    return I;
}

// The culls' bounding-sphere and normal-cone tests take an instance's R for a rotation (the sphere's radius is radius * |s|, the cone's
// axis is turned by R).  R is a product of matrices built from zr_sincos: inside its domain a rotation to 1e-6, outside it (zr_math.h)
// any finite matrix or NaN.  Columns orthonormal within 1e-4 - well inside the tests' margins (the radius is inflated by 1e-3, the cone
// widened by 0.02) - else the record gets no sphere or cone test; the box test is affine in R and holds for any matrix.
__device__ __forceinline__ bool is_rotation(const float* R)
{
    const zf3 a = zr3(R[0], R[1], R[2]), b = zr3(R[3], R[4], R[5]), c = zr3(R[6], R[7], R[8]);
    const float T = 1e-4f;
    return __builtin_fabsf(zr_dot(a, a) - 1.0f) <= T && __builtin_fabsf(zr_dot(b, b) - 1.0f) <= T && __builtin_fabsf(zr_dot(c, c) - 1.0f) <= T &&
           __builtin_fabsf(zr_dot(a, b)) <= T && __builtin_fabsf(zr_dot(a, c)) <= T && __builtin_fabsf(zr_dot(b, c)) <= T;     // NaN: false
}

// Base.vert:26 / BaseInstanced.vert:70 / Shadowmap*.vert: object-space position fed to PVM
__device__ __forceinline__ zf3 vs_position(zf3 p, const ZrInstance& I, bool instanced)
{
    if (!instanced) return p;
    zf3 q = zr_rowvec_mat3(p * I.s, I.R);
    return zr3(q.x + I.t[0], q.y + I.t[1], q.z + I.t[2]);
}
// outNormal = (M * vec4(normalize(n), 1)).xyz [* mat3(rotMat)] — the w = 1 is the engine's own (Base.vert:29)
__device__ __forceinline__ zf3 vs_normal(zf3 n, const ZrInstance& I, bool instanced, const float* M)
{
    zf4 mn = zr_mat4_point(M, zr_normalize(n));
    zf3 r = zr3(mn.x, mn.y, mn.z);
    return instanced ? zr_rowvec_mat3(r, I.R) : r;
}

// bit0 non-finite, bits1-6 outside {x<-w, x>w, y<-w, y>w, z<0, z>w}, bit7 needs clipping
__device__ __forceinline__ uint32_t vertex_flags(zf4 c)
{
    const float FM = 3.402823466e38f;
    uint32_t f = 0;
    if (!(__builtin_fabsf(c.x) <= FM && __builtin_fabsf(c.y) <= FM && __builtin_fabsf(c.z) <= FM && __builtin_fabsf(c.w) <= FM)) f |= 1u;
    if (c.x < -c.w) f |= 2u;
    if (c.x > c.w) f |= 4u;
    if (c.y < -c.w) f |= 8u;
    if (c.y > c.w) f |= 16u;
    if (c.z < 0.0f) f |= 32u;
    if (c.z > c.w) f |= 64u;
    float g = ZR_GUARD * c.w;
    if (c.z < 0.0f || !(c.w > 0.0f) || __builtin_fabsf(c.x) > g || __builtin_fabsf(c.y) > g) f |= 128u;
    return f;
}
// 0 discard, 1 fast path, 2 clip path
__device__ __forceinline__ int classify(uint32_t f0, uint32_t f1, uint32_t f2)
{
    if ((f0 | f1 | f2) & 1u) return 0;
    if (f0 & f1 & f2 & 0x7Eu) return 0;
    return ((f0 | f1 | f2) & 128u) ? 2 : 1;
}

// float -> int of a snapped coordinate.  A corner that classify() lets through has |x|, |y| <= 4 w, but for a denormal w the reciprocal
// below is +inf and the products are +-inf or NaN; a cast of those is undefined (x86 and gfx950 give different values).  Clamping to the
// ints a float can hold defines it: NaN -> -2^31 (zr_math.h: max(NaN, a) = a), +-inf and anything beyond -> -2^31 / 2^31 - 128.
__device__ __forceinline__ int snap_to_int(float f) { return (int)__builtin_fminf(__builtin_fmaxf(f, -2147483648.0f), 2147483520.0f); }
__device__ __forceinline__ SV project(zf4 c, float hw, float hh)
{
    SV s;
    s.rw = 1.0f / c.w;                     // one IEEE reciprocal, then multiplies (the perspective divide)
    const float nx = c.x * s.rw, ny = c.y * s.rw;
    const float xs = __builtin_fmaf(nx, hw, hw), ys = __builtin_fmaf(ny, hh, hh);
    s.X = snap_to_int(__builtin_floorf(__builtin_fmaf(xs, 256.0f, 0.5f)));
    s.Y = snap_to_int(__builtin_floorf(__builtin_fmaf(ys, 256.0f, 0.5f)));
    s.z = c.z * s.rw;
    return s;
}

// ------------------------------------------------------------------------------------------------ steps the geometry kernels share

// A rectangle of tiles in one word: tx0 | ty0 << 8 | tx1 << 16 | ty1 << 24 (the cull's rects, a triangle's tiles, a slow triangle's reach).
struct TileRect { uint32_t tx0, ty0, tx1, ty1; };
__device__ __forceinline__ TileRect rect_unpack(uint32_t r) { TileRect R; R.tx0 = r & 255u; R.ty0 = (r >> 8) & 255u; R.tx1 = (r >> 16) & 255u; R.ty1 = r >> 24; return R; }
// ... of the tiles a pixel box (inside the target) reaches
__device__ __forceinline__ uint32_t rect_of_pixels(int px0, int py0, int px1, int py1)
{
    return (uint32_t)(px0 / TILE) | (uint32_t)(py0 / TILE) << 8 | (uint32_t)(px1 / TILE) << 16 | (uint32_t)(py1 / TILE) << 24;
}
__device__ __forceinline__ bool rect_has(uint32_t r, int tx, int ty)
{
    return (int)(r & 255u) <= tx && tx <= (int)((r >> 16) & 255u) && (int)((r >> 8) & 255u) <= ty && ty <= (int)(r >> 24);
}

// The LDS histogram over the tiles of the shadow map (k_bin_count, k_bin_fill; 1024 threads): zeroed, then every listed rect adds one
// to each of its tiles (the callers' barriers stand between the two and after; a culled item has no rect to add).
__device__ __forceinline__ void hist_clear(uint32_t* hist, uint32_t n_tiles)
{
    for (uint32_t i = threadIdx.x; i < n_tiles; i += 1024u) hist[i] = 0;
}
__device__ __forceinline__ void hist_add_rect(uint32_t* hist, const TileRect& R, uint32_t tiles_x)
{
    for (uint32_t ty = R.ty0; ty <= R.ty1; ++ty)
        for (uint32_t tx = R.tx0; tx <= R.tx1; ++tx) atomicAdd(&hist[ty * tiles_x + tx], 1u);
}

// One meshlet-instance as the self-contained record the rasterising waves start from (ZrBinEntry): from the parts of the meshlet's
// header (the cull has them at hand), or from work item w alone: find the object, split into instance and meshlet, load the header.
__device__ __forceinline__ ZrBinEntry bin_entry(const ZrObject* O, uint32_t inst_i, const float4* mpos, uint32_t tri_base, uint32_t vcount, uint32_t tcount,
                                               uint32_t instanced)
{
    ZrBinEntry be;
    be.mpos = mpos; be.mtri = O->mtri + tri_base; be.inst = O->inst + inst_i;
    be.counts = vcount | tcount << 8 | (instanced ? 1u << 16 : 0u);
    be.prim_base = O->prim_base + inst_i * O->n_tris;
    return be;
}
__device__ __forceinline__ ZrBinEntry bin_entry(const ZrObject* objs, int n_objects, uint32_t w)
{
    const ZrObject* __restrict__ O = objs + find_object_work(objs, n_objects, w);
    const uint32_t local = w - O->work_base;
    const uint32_t inst_i = local / O->n_meshlets, m = local - inst_i * O->n_meshlets;
    const XkMeshlet* __restrict__ ml = O->meshlets + m;
    const uint4 mh = ld_global((const uint4*)ml);            // VertexOffset, VertexCount, TriangleOffset, TriangleCount
    return bin_entry(O, inst_i, O->mpos + mh.x, ld_global(&ml->BindlessContext), mh.y, mh.w, O->instanced);
}

// The head of a meshlet in a rasterising wave (k_raster_chunks, k_geom), from its record (wave-uniform): both rounds' triangle words, the
// lane's vertex and the instance are requested together, before anything waits; the vertex is transformed.  Almost every meshlet has no
// vertex outside the frustum at all: the callers take one wave-wide vote over ten comparisons (each a 64-lane mask by itself); only a
// FLAGGED meshlet pays for the per-vertex flag words and the per-triangle classification.  (The vote, the flags and the projection stay
// with the callers, around what each stages of its vertex: inlined from here the compiler folds their branches differently.)
struct MeshletHead {
    const float4* mp; ZrInstance I; bool instanced;      // (what a slow triangle's vertices are transformed from again)
    uint32_t vcount, tcount, pbase;
    uint2 tri_w[2];
    zf4 c;              // lanes below vcount: the lane's vertex in clip space
};
__device__ __forceinline__ MeshletHead meshlet_head(const float* PVM, const ZrBinEntry& be, uint32_t lane)
{
    MeshletHead H;
    H.mp = be.mpos; H.pbase = be.prim_base;
    const uint2* tw = be.mtri;
    H.vcount = be.counts & 255u; H.tcount = (be.counts >> 8) & 255u;
    H.instanced = (be.counts >> 16) & 1u;
    H.tri_w[0] = lane < H.tcount ? ld_global(tw + lane) : make_uint2(0u, 0u);
    H.tri_w[1] = lane + WAVE < H.tcount ? ld_global(tw + lane + WAVE) : make_uint2(0u, 0u);
    const float4 pp = lane < H.vcount ? ld_global(H.mp + lane) : make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    H.I = ld_record(be.inst);

    lds_fence();   // this wave's previous readers are done with its staging area
    H.c = zr_mat4_point(PVM, vs_position(zr3(pp.x, pp.y, pp.z), H.I, H.instanced));
    return H;
}

// What a colour leaves a shader as: the gamma every .frag applies (pow(c, 0.4545) per channel), the R8G8B8A8_UNORM word with alpha 1
__device__ __forceinline__ zf3 gamma3(zf3 c) { return zr3(zr_pow(c.x, 0.4545f), zr_pow(c.y, 0.4545f), zr_pow(c.z, 0.4545f)); }
__device__ __forceinline__ uint32_t pack_rgb8(zf3 c) { return zr_unorm(c.x, 255.0f) | zr_unorm(c.y, 255.0f) << 8 | zr_unorm(c.z, 255.0f) << 16 | 255u << 24; }

// Multi-GPU ownership of a tile (zelda_render.h: zr_tile_owner)
__device__ __forceinline__ uint32_t tile_owner(uint32_t tx, uint32_t ty, uint32_t world)
{
    return ((tx >> ZR_SUPERTILE_SHIFT) + (ty >> ZR_SUPERTILE_SHIFT) * ZR_SUPERTILE_SKEW) % world;
}

__device__ __forceinline__ int imin3(int a, int b, int c) { return min(a, min(b, c)); }
__device__ __forceinline__ int imax3(int a, int b, int c) { return max(a, max(b, c)); }

// Wave-wide reductions on the DPP network (no LDS round trips): an inclusive scan over each row of 16 lanes (row_shr 1, 2, 4,
// 8), then row_bcast15 / row_bcast31 fold the rows; lane 63 holds the result, which is broadcast through an SGPR.
// `idn` is the operation's identity (what lanes without a source contribute).
#define ZR_DPP_STEP(OP, ctrl, rmask) r = OP(r, __builtin_amdgcn_update_dpp(idn, r, ctrl, rmask, 0xF, false))
#define ZR_WAVE_REDUCE(OP)                                                                 \
    int r = v;                                                                              \
    ZR_DPP_STEP(OP, 0x111, 0xF); ZR_DPP_STEP(OP, 0x112, 0xF); ZR_DPP_STEP(OP, 0x114, 0xF);   \
    ZR_DPP_STEP(OP, 0x118, 0xF); ZR_DPP_STEP(OP, 0x142, 0xA); ZR_DPP_STEP(OP, 0x143, 0xC);   \
    return __builtin_amdgcn_readlane(r, 63)
__device__ __forceinline__ int op_min(int a, int b) { return min(a, b); }
__device__ __forceinline__ int op_max(int a, int b) { return max(a, b); }
__device__ __forceinline__ int op_or(int a, int b) { return a | b; }
__device__ __forceinline__ int op_and(int a, int b) { return a & b; }
__device__ __forceinline__ int op_add(int a, int b) { return a + b; }
__device__ __forceinline__ int wave_min(int v) { const int idn = 0x7FFFFFFF; ZR_WAVE_REDUCE(op_min); }
__device__ __forceinline__ int wave_max(int v) { const int idn = (int)0x80000000; ZR_WAVE_REDUCE(op_max); }
__device__ __forceinline__ int wave_sum(int v) { const int idn = 0; ZR_WAVE_REDUCE(op_add); }
__device__ __forceinline__ uint32_t wave_or(uint32_t u) { const int idn = 0, v = (int)u; ZR_WAVE_REDUCE(op_or); }
__device__ __forceinline__ uint32_t wave_and(uint32_t u) { const int idn = -1, v = (int)u; ZR_WAVE_REDUCE(op_and); }
typedef short short2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int op_pkmin(int a, int b) { short2_t x, y; __builtin_memcpy(&x, &a, 4); __builtin_memcpy(&y, &b, 4); x = __builtin_elementwise_min(x, y); int r; __builtin_memcpy(&r, &x, 4); return r; }
__device__ __forceinline__ int op_pkmax(int a, int b) { short2_t x, y; __builtin_memcpy(&x, &a, 4); __builtin_memcpy(&y, &b, 4); x = __builtin_elementwise_max(x, y); int r; __builtin_memcpy(&r, &x, 4); return r; }
// two int16 lanes per register: one reduction for (x, y) pairs
__device__ __forceinline__ int wave_pkmin16(int v) { const int idn = 0x7FFF7FFF; ZR_WAVE_REDUCE(op_pkmin); }
__device__ __forceinline__ int wave_pkmax16(int v) { const int idn = (int)0x80008000; ZR_WAVE_REDUCE(op_pkmax); }
__device__ __forceinline__ int clamp16(int v) { return min(max(v, -32768), 32767); }
__device__ __forceinline__ int op_fmin(int a, int b) { return (int)zr_f2u(__builtin_fminf(zr_u2f((uint32_t)a), zr_u2f((uint32_t)b))); }
__device__ __forceinline__ int op_fmax(int a, int b) { return (int)zr_f2u(__builtin_fmaxf(zr_u2f((uint32_t)a), zr_u2f((uint32_t)b))); }
__device__ __forceinline__ float wave_fmin(float f) { const int idn = 0x7F800000, v = (int)zr_f2u(f); return zr_u2f((uint32_t)[&]() { ZR_WAVE_REDUCE(op_fmin); }()); }
__device__ __forceinline__ float wave_fmax(float f) { const int idn = (int)0xFF800000, v = (int)zr_f2u(f); return zr_u2f((uint32_t)[&]() { ZR_WAVE_REDUCE(op_fmax); }()); }

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)      // inclusive prefix sum over the wave's lanes (rows on the DPP network, then across)
{
    const int idn = 0;
    int r = (int)v;
    ZR_DPP_STEP(op_add, 0x111, 0xF); ZR_DPP_STEP(op_add, 0x112, 0xF); ZR_DPP_STEP(op_add, 0x114, 0xF); ZR_DPP_STEP(op_add, 0x118, 0xF);
    ZR_DPP_STEP(op_add, 0x142, 0xA); ZR_DPP_STEP(op_add, 0x143, 0xC);
    return (uint32_t)r;
}
__device__ __forceinline__ float lane_bcast(float v, uint32_t src) { return zr_u2f((uint32_t)__builtin_amdgcn_readlane((int)zr_f2u(v), (int)src)); }
__device__ __forceinline__ uint32_t lane_bcast(uint32_t v, uint32_t src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src); }

// The calling thread's four pixels (px .. px + 3, py) of a row-major W x H plane (zr_delta.hip, zr_scale.hip); 0 where they lie outside
// it.  VEC: W % 4 == 0 and px % 4 == 0, so px < W puts all four inside and the address on a 16-byte boundary.
template <bool VEC> __device__ __forceinline__ uint4 plane_load4(const uint32_t* __restrict__ plane, uint32_t W, uint32_t H, uint32_t px, uint32_t py)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (py >= H || px >= W) return v;
    const uint32_t* p = plane + (size_t)py * W + px;
    if (VEC) return *reinterpret_cast<const uint4*>(p);
    v.x = p[0];
    if (px + 1u < W) v.y = p[1];
    if (px + 2u < W) v.z = p[2];
    if (px + 3u < W) v.w = p[3];
    return v;
}
template <bool VEC> __device__ __forceinline__ void plane_store4(uint32_t* __restrict__ plane, uint32_t W, uint32_t H, uint32_t px, uint32_t py, uint4 v)
{
    if (py >= H || px >= W) return;
    uint32_t* p = plane + (size_t)py * W + px;
    if (VEC) { *reinterpret_cast<uint4*>(p) = v; return; }
    p[0] = v.x;
    if (px + 1u < W) p[1] = v.y;
    if (px + 2u < W) p[2] = v.z;
    if (px + 3u < W) p[3] = v.w;
}

// Conservative occlusion test of one meshlet-instance against the pyramid: true when every pixel of its snapped bounding box
// already holds a depth smaller than the least depth the meshlet can produce, i.e. its fragments would all fail LESS.
__device__ __forceinline__ bool hiz_occluded(const ZrHiz& Z, uint2 pr, float zmin)
{
    if (!(zmin >= 0.0f)) return false;
    const uint32_t x0 = pr.x & 0xFFFFu, y0 = pr.x >> 16, x1 = pr.y & 0xFFFFu, y1 = pr.y >> 16;
    uint32_t l = 0;                                        // 0: the 4 x 4 pixel level, 1..4: lvl[0..3]
    // the finest level at which the box spans at most 4 texels per axis
    while (l < 4u && (((x1 >> (2u + l)) - (x0 >> (2u + l))) > 3u || ((y1 >> (2u + l)) - (y0 >> (2u + l))) > 3u)) ++l;
    const uint32_t sh = 2u + l;
    const uint32_t tx0 = x0 >> sh, ty0 = y0 >> sh, tx1 = x1 >> sh, ty1 = y1 >> sh;
    if (tx1 - tx0 > 3u || ty1 - ty0 > 3u) return false;     // wider than 4x4 texels of the coarsest level: not tested
    const float* __restrict__ L = l == 0u ? Z.fine : Z.lvl[l - 1u];
    const uint32_t hw = l == 0u ? Z.fw : Z.hw[l - 1u];
    // 16 independent loads (clamped repeats at the far edges) instead of a data-dependent loop: one memory latency, not sixteen
    float hmax = 0.0f;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j)
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i)
            hmax = __builtin_fmaxf(hmax, L[(size_t)min(ty0 + j, ty1) * hw + min(tx0 + i, tx1)]);
    // fragment depths are clamped to their triangle's vertex depths (shade_key), so zmin bounds them exactly
    return zmin > hmax;
}

// Shape of the per-pixel kernels' grids (A/B'd on the whole two-lane frame, not on the kernel alone: what counts is what the pass
// leaves to the other lane while it runs).  Pixels per thread 1 instead of 4: + 3.5 % (the pass itself takes LONGER beside the camera
// lane, 123 -> 187 us, and the camera lane's short kernels stop starving: hiz 80 -> 40 us); 512-thread workgroups for the lighting
// pass: + 1 % more (128 threads: - 8 %, 1 024: - 2 %; single-wave workgroups at 4 pixels per thread: - 3 %).  One pixel per thread
// is also what a rank of a multi-GPU job needs, whose few tiles would otherwise fill a quarter of the machine.
#ifndef ZR_LIGHT_TB
#define ZR_LIGHT_TB 512
#endif
#ifndef ZR_LIGHT_WAVES
#define ZR_LIGHT_WAVES 6             // waves per SIMD k_lighting is compiled for (see the note at the kernel)
#endif
// ... and the same two for the variant that reads a pixel's standing terms from the kept plane (k_lighting, ZR_LIGHT_KEPT): it holds no PCF
// rows and no cubemap texels, so it fits more waves (DESIGN.md section 7 has the variants tried)
#ifndef ZR_LIGHT_KEPT_TB
#define ZR_LIGHT_KEPT_TB 512
#endif
#ifndef ZR_LIGHT_KEPT_WAVES
#define ZR_LIGHT_KEPT_WAVES 8
#endif
// What k_lighting_rest takes from the fill's records instead of the GBuffer: the tile light list's box (k_lighting rebuilds it from its
// pixels' scene_color and gD, wave reductions and an LDS merge) and which pixels are empty, whose 24 GBuffer bytes it does not fetch.
// How it is set up: a light's eight dwords are read before any of them is compared - the tile list's test from an LDS copy staged with
// the tables, the light loop by one scalar load - and a part's eight records arrive as one vector load per lane behind one wait, the box
// by row reductions on the DPP network.  That last one keeps its other arm (0: a scalar load and a wait per record, in a loop): the
// control build of tests/test_kernel_table_rest_setup.py.  (DESIGN.md section 7 has each of these measured on its own; App. A what was
// measured with them and taken out again.)
#ifndef ZR_REST_RECORDS_ONE_TRIP
#define ZR_REST_RECORDS_ONE_TRIP 1
#endif
#ifndef ZR_PIXELS_PER_THREAD
#define ZR_PIXELS_PER_THREAD 1     // of k_resolve_gbuffer and k_lighting: 1, 2 or 4 (a tile is 1 024 pixels; workgroups per tile follow)
#endif
static_assert(TILE_PIX / ZR_PIXELS_PER_THREAD >= ZR_LIGHT_KEPT_TB, "a tile's threads must fill at least one workgroup");
static_assert(TILE_PIX / ZR_PIXELS_PER_THREAD >= ZR_LIGHT_TB && TILE_PIX / ZR_PIXELS_PER_THREAD >= 256, "a tile's threads must fill at least one workgroup");
#ifndef ZR_RESOLVE_TB
#define ZR_RESOLVE_TB 256
#endif
