// zr_texture_update.hip — material textures replaced between frames (zr_object_set_texture, zr_object_update_texture_async).
//
// A slot's new level 0 arrives in device memory; its mip chain - and, when the object has the packed form, the slot's bytes of the packed
// chain - is rewritten in place, on the update's stream:
//   k_tex_level0   a lane per texel: the new image into level 0
//   k_tex_mip      a lane per destination texel: level l from level l - 1 (four 32-bit loads, one 32-bit store)
//   k_tex_tail     one workgroup: from the first level of at most 64 x 64 texels on, every remaining level through LDS
// The statement is build_mip_chain (zr_scene.cpp), byte for byte: the same fmaf sequence and clamped indices; decode through the two
// 256-entry tables the resolve uses; the linear encode is zr_unorm, the sRGB encode a search of the host's own thresholds (zr_srgb.h) -
// no pow and no division on the device (the levels' steps come as the host's quotients).  Ordering against frames: the host file.
#include "zr_dev.h"

#define ZR_TEX_THREADS 256u
#define ZR_TEX_TAIL 64u                      // k_tex_tail computes the levels of at most this edge

struct TexTables { float dec_rgb[256], dec_a[256], thr[256]; };      // channel 0..2 / channel 3 decode; the encode thresholds

// (ZR_TEX_THREADS == 256: an entry per lane)
__device__ __forceinline__ void stage_tables(TexTables& T, const ZrTexUpdate& U)
{
    const uint32_t t = threadIdx.x;
    T.dec_rgb[t] = U.srgb ? U.srgb_lut[t] : U.unorm_lut[t];
    T.dec_a[t] = U.unorm_lut[t];
    T.thr[t] = U.srgb_thr[t];
    __syncthreads();
}

// srgb_encode8(v): how many of thr[1 .. 255] v reaches (8 steps; thr[0] = -inf is never asked)
__device__ __forceinline__ uint32_t srgb_encode_thr(float v, const float* thr)
{
    uint32_t k = 0;
#pragma unroll
    for (uint32_t bit = 128u; bit; bit >>= 1) if (v >= thr[k + bit]) k += bit;
    return k;
}

__device__ __forceinline__ int tex_idx_clamp(float f, int hi) { f = __builtin_fminf(__builtin_fmaxf(f, 0.0f), (float)hi); return (int)f; }

// texel (x, y) of a level from its sw x sh source level (global memory or LDS): build_mip_chain's inner loop
__device__ __forceinline__ uint32_t mip_texel(const uint32_t* src, uint32_t sw, uint32_t sh, float kx, float ky, uint32_t x, uint32_t y,
                                              bool srgb, const TexTables& T)
{
    const float fu = __builtin_fmaf((float)x + 0.5f, kx, -0.5f), fv = __builtin_fmaf((float)y + 0.5f, ky, -0.5f);
    const float fx = __builtin_floorf(fu), fy = __builtin_floorf(fv), a = fu - fx, b = fv - fy;
    const int x0 = tex_idx_clamp(fx, (int)sw - 1), x1 = tex_idx_clamp(fx + 1.0f, (int)sw - 1);
    const int y0 = tex_idx_clamp(fy, (int)sh - 1), y1 = tex_idx_clamp(fy + 1.0f, (int)sh - 1);
    const uint32_t p00 = src[(uint32_t)y0 * sw + (uint32_t)x0], p10 = src[(uint32_t)y0 * sw + (uint32_t)x1];
    const uint32_t p01 = src[(uint32_t)y1 * sw + (uint32_t)x0], p11 = src[(uint32_t)y1 * sw + (uint32_t)x1];
    uint32_t out = 0;
#pragma unroll
    for (uint32_t ch = 0; ch < 4u; ++ch) {
        const float* dec = ch < 3u ? T.dec_rgb : T.dec_a;
        const float t00 = dec[(p00 >> (8u * ch)) & 255u], t10 = dec[(p10 >> (8u * ch)) & 255u];
        const float t01 = dec[(p01 >> (8u * ch)) & 255u], t11 = dec[(p11 >> (8u * ch)) & 255u];
        const float top = __builtin_fmaf(a, t10 - t00, t00), bot = __builtin_fmaf(a, t11 - t01, t01);
        const float v = __builtin_fmaf(b, bot - top, top);
        const uint32_t e = (srgb && ch < 3u) ? srgb_encode_thr(v, T.thr) : (zr_unorm(v, 255.0f) & 255u);
        out |= e << (8u * ch);
    }
    return out;
}

// the slot's bytes of packed texel `texel` (the bytes beside them belong to other slots: byte stores)
__device__ __forceinline__ void put_packed(const ZrTexUpdate& U, size_t texel, uint32_t px)
{
    if (!U.packed) return;
    uint8_t* d = U.packed + texel * 16u + U.pk_ch;
    for (uint32_t k = 0; k < U.pk_n; ++k) d[k] = (uint8_t)(px >> (8u * k));
}

__device__ __forceinline__ uint32_t level_edge(uint32_t e, uint32_t l) { const uint32_t v = e >> l; return v ? v : 1u; }

__global__ __launch_bounds__(ZR_TEX_THREADS) void k_tex_level0(ZrTexUpdate U, const uint32_t* __restrict__ src)
{
    const size_t i = (size_t)blockIdx.x * ZR_TEX_THREADS + threadIdx.x;
    if (i >= (size_t)U.w * U.h) return;
    const uint32_t px = src[i];
    U.chain[i] = px;
    put_packed(U, i, px);
}

__global__ __launch_bounds__(ZR_TEX_THREADS) void k_tex_mip(ZrTexUpdate U, uint32_t l)
{
    __shared__ TexTables T;
    stage_tables(T, U);
    const uint32_t sw = level_edge(U.w, l - 1u), sh = level_edge(U.h, l - 1u), dw = level_edge(U.w, l), dh = level_edge(U.h, l);
    const uint32_t i = blockIdx.x * ZR_TEX_THREADS + threadIdx.x;
    if (i >= dw * dh) return;
    const uint32_t px = mip_texel(U.chain + U.off[l - 1u], sw, sh, U.kx[l], U.ky[l], i % dw, i / dw, U.srgb != 0u, T);
    U.chain[U.off[l] + i] = px;
    put_packed(U, (size_t)U.off[l] + i, px);
}

// levels first .. levels - 1; level `first` (at most ZR_TEX_TAIL on either edge) from level first - 1 in global memory, the rest from LDS
__global__ __launch_bounds__(ZR_TEX_THREADS) void k_tex_tail(ZrTexUpdate U, uint32_t first)
{
    __shared__ TexTables T;
    __shared__ uint32_t buf_a[ZR_TEX_TAIL * ZR_TEX_TAIL], buf_b[ZR_TEX_TAIL * ZR_TEX_TAIL / 4u];      // levels first, first + 2 .. / first + 1, first + 3 ..
    stage_tables(T, U);
    const uint32_t* src = U.chain + U.off[first - 1u];
    uint32_t* dst = buf_a;
    uint32_t sw = level_edge(U.w, first - 1u), sh = level_edge(U.h, first - 1u);
    for (uint32_t l = first; l < U.levels; ++l) {
        const uint32_t dw = level_edge(U.w, l), dh = level_edge(U.h, l);
        const uint32_t cap = dst == buf_a ? ZR_TEX_TAIL * ZR_TEX_TAIL : ZR_TEX_TAIL * ZR_TEX_TAIL / 4u;
        for (uint32_t i = threadIdx.x; i < dw * dh && i < cap; i += ZR_TEX_THREADS) {
            const uint32_t px = mip_texel(src, sw, sh, U.kx[l], U.ky[l], i % dw, i / dw, U.srgb != 0u, T);
            dst[i] = px;
            U.chain[U.off[l] + i] = px;
            put_packed(U, (size_t)U.off[l] + i, px);
        }
        __syncthreads();      // level l is whole before level l + 1 reads it - and level l - 1 has been read before l + 1 overwrites it
        src = dst; dst = dst == buf_a ? buf_b : buf_a; sw = dw; sh = dh;
    }
}

// the tail's first level: the first whose edges are both at most ZR_TEX_TAIL - but not level 0, which is the new image
static uint32_t tail_first(const ZrTexUpdate& U)
{
    uint32_t l = 1;
    while (l < U.levels && std::max(std::max(U.w >> l, U.h >> l), 1u) > ZR_TEX_TAIL) ++l;
    return l;
}

void zr_launch_texture_update(const ZrTexUpdate& U, const uint32_t* src, hipStream_t s)
{
    const size_t n0 = (size_t)U.w * U.h;
    if (n0 == 0 || U.levels == 0 || U.levels > 16u) return;
    hipLaunchKernelGGL(k_tex_level0, dim3((uint32_t)((n0 + ZR_TEX_THREADS - 1u) / ZR_TEX_THREADS)), dim3(ZR_TEX_THREADS), 0, s, U, src);
    const uint32_t first = tail_first(U);
    for (uint32_t l = 1; l < first; ++l) {
        const uint32_t n = std::max(U.w >> l, 1u) * std::max(U.h >> l, 1u);
        hipLaunchKernelGGL(k_tex_mip, dim3((n + ZR_TEX_THREADS - 1u) / ZR_TEX_THREADS), dim3(ZR_TEX_THREADS), 0, s, U, l);
    }
    if (first < U.levels) hipLaunchKernelGGL(k_tex_tail, dim3(1), dim3(ZR_TEX_THREADS), 0, s, U, first);
}
