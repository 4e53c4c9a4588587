// zr_mesh_update.hip — vertex updates between frames (zr_mesh_set_vertices, zr_mesh_update_vertices_async).
//
// An updated mesh keeps, on the device: its raw XkVertex array (what the update calls write) and two sets of everything a frame reads
// that depends on vertex values (ZrMeshSet: one per frame parity, read through the draw table of that parity).  k_vertex_scatter writes
// raw values; at the head of the next frame of each parity the refit rebuilds that parity's whole set from them - there is no per-vertex
// dirty tracking, a refit costs the mesh - in three launches on the frame's first stream:
//   k_mesh_refit        a wave per meshlet: mpos, mbox, the meshlet's rtris, its sphere and cone; the mesh's box (atomics)
//   k_mesh_refit_verts  a lane per vertex: verts, rverts; the greatest distance from the box centre (atomic)
//   k_table_set_mesh    one workgroup: the set's pointers and the whole-mesh sphere into every draw record that uses the mesh
// Which sets are stale, and the ordering against updates and frames, live on the host (zr_mesh_update_host.cpp).
#include "zr_dev.h"
#include "zr_bounds.h"

// vertices [first, first + n) of raw from src, dword by dword (src is only 4-byte aligned; an XkVertex is 11 dwords)
__global__ void k_vertex_scatter(const uint32_t* __restrict__ src, uint32_t* __restrict__ raw, uint32_t first, uint32_t n, uint32_t n_verts)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (size_t)n * 11u) return;
    const size_t k = (size_t)first * 11u + j;
    if (k < (size_t)n_verts * 11u) raw[k] = src[j];
}

// the resolve's record of one vertex: upload_mesh's statement (zr_scene.cpp), bit for bit
__device__ __forceinline__ void put_rvertex(ZrRVertex* dst, const XkVertex& x)
{
    const zf3 n = zr_normalize(zr3(x.Normal[0], x.Normal[1], x.Normal[2]));
    float4* d = (float4*)dst;
    d[0] = make_float4(x.Position[0], x.Position[1], x.Position[2], x.TexCoord[0]);
    d[1] = make_float4(n.x, n.y, n.z, x.TexCoord[1]);
}
__device__ __forceinline__ XkVertex load_vertex(const XkVertex* p)
{
    XkVertex v;
    const uint32_t* s = (const uint32_t*)p;
    uint32_t* d = (uint32_t*)&v;
#pragma unroll
    for (int i = 0; i < 11; ++i) d[i] = s[i];
    return v;
}
// floats as integers of the same order (atomicMin / atomicMax on them)
__device__ __forceinline__ uint32_t ordered(float f) { const uint32_t u = zr_f2u(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float unordered(uint32_t u) { return zr_u2f((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

#define ZR_REFIT_WAVES 4u
struct RefitCorner {        // corner k of the meshlet's triangle t, from the words staged in LDS
    const uint32_t* words;
    __device__ uint32_t operator()(uint32_t t, uint32_t k) const { return (words[t] >> (8u * k)) & 255u; }
};

__global__ __launch_bounds__(ZR_REFIT_WAVES * WAVE) void k_mesh_refit(ZrMeshState S, uint32_t par)
{
    // the meshlet's vertices and triangle words, for the one lane that walks them serially in float64 (zr_meshlet_bounds_of)
    __shared__ XkVertex lv[ZR_REFIT_WAVES][64];
    __shared__ uint32_t lt[ZR_REFIT_WAVES][128];
    __shared__ uint32_t ident[64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    if (threadIdx.x < 64u) ident[threadIdx.x] = threadIdx.x;
    __syncthreads();
    const uint32_t m = blockIdx.x * ZR_REFIT_WAVES + wv;
    if (m >= S.n_meshlets) return;
    const ZrMeshSet D = S.set[par];
    XkMeshlet* ml = D.meshlets + m;
    const uint32_t vo = ml->VertexOffset, vc = min(ml->VertexCount, 64u), tc = min(ml->TriangleCount, 128u), tb = ml->BindlessContext;
    const float INF = __builtin_inff();
    float x = INF, y = INF, z = INF, X = -INF, Y = -INF, Z = -INF;
    if (lane < vc) {
        const uint32_t vi = min(S.mverts[vo + lane], S.n_verts - 1u);
        const float* p = S.raw[vi].Position;
        x = X = p[0]; y = Y = p[1]; z = Z = p[2];
        D.mpos[vo + lane] = make_float4(x, y, z, 1.0f);
        lv[wv][lane].Position[0] = x; lv[wv][lane].Position[1] = y; lv[wv][lane].Position[2] = z;
    }
    // (fminf / fmaxf: a NaN coordinate drops out, as in upload_mesh's std::min / std::max against a finite or infinite bound)
    x = wave_fmin(x); y = wave_fmin(y); z = wave_fmin(z); X = wave_fmax(X); Y = wave_fmax(Y); Z = wave_fmax(Z);
    for (uint32_t t = lane; t < tc; t += WAVE) {
        const uint2 w = S.mtri[tb + t];
        lt[wv][t] = w.x;
        if (w.y < S.n_tris)
            for (uint32_t k = 0; k < 3u; ++k) {
                const uint32_t vi = min(S.indices[3u * w.y + k], S.n_verts - 1u);
                put_rvertex(D.rtris + 3u * (size_t)w.y + k, load_vertex(S.raw + vi));
            }
    }
    lds_fence();
    if (lane == 0) {
        D.mbox[2u * m] = make_float4(x, y, z, 0.0f); D.mbox[2u * m + 1u] = make_float4(X, Y, Z, 0.0f);
        atomicMin(D.acc + 0, ordered(x)); atomicMin(D.acc + 1, ordered(y)); atomicMin(D.acc + 2, ordered(z));
        atomicMax(D.acc + 3, ordered(X)); atomicMax(D.acc + 4, ordered(Y)); atomicMax(D.acc + 5, ordered(Z));
        XkMeshlet b = *ml;
        zr_meshlet_bounds_of(lv[wv], ident, vc, RefitCorner{ lt[wv] }, tc, &b);
        *ml = b;
    }
}

__global__ __launch_bounds__(256) void k_mesh_refit_verts(ZrMeshState S, uint32_t par)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const ZrMeshSet D = S.set[par];
    double dist = 0.0;
    if (i < S.n_verts) {
        const XkVertex v = load_vertex(S.raw + i);
        uint32_t* d = (uint32_t*)(D.verts + i);
        const uint32_t* s = (const uint32_t*)&v;
#pragma unroll
        for (int k = 0; k < 11; ++k) d[k] = s[k];
        put_rvertex(D.rverts + i, v);
        // the box is final: k_mesh_refit ran ahead of this kernel on the stream
        float c[3];
        for (int a = 0; a < 3; ++a) c[a] = (float)(((double)unordered(D.acc[a]) + (double)unordered(D.acc[3 + a])) * 0.5);
        const double dx = (double)v.Position[0] - c[0], dy = (double)v.Position[1] - c[1], dz = (double)v.Position[2] - c[2];
        dist = sqrt(dx * dx + dy * dy + dz * dz);
    }
    for (int o = 32; o > 0; o >>= 1) dist = fmax(dist, __shfl_xor(dist, o));      // (fmax: a NaN distance drops out)
    if ((threadIdx.x & 63u) == 0 && dist > 0.0) atomicMax((unsigned long long*)(D.acc + 6), (unsigned long long)__double_as_longlong(dist));
}

// every draw record of the table that uses the mesh (its shared index buffer names it): the set's pointers, the whole-mesh sphere -
// box centre + greatest distance, inflated as upload_mesh inflates its own.  Then the reduction's cells are reset for the next refit.
__global__ void k_table_set_mesh(ZrObject* __restrict__ tab, uint32_t n_objs, ZrMeshState S, uint32_t par)
{
    const ZrMeshSet D = S.set[par];
    float c[3];
    for (int a = 0; a < 3; ++a) c[a] = (float)(((double)unordered(D.acc[a]) + (double)unordered(D.acc[3 + a])) * 0.5);
    const double r = __longlong_as_double((long long)*(const unsigned long long*)(D.acc + 6));
    const float radius = (float)(r * 1.0001) + 1e-30f;
    for (uint32_t i = threadIdx.x; i < n_objs; i += blockDim.x) {
        ZrObject* O = tab + i;
        if (O->indices != S.indices) continue;
        O->verts = D.verts; O->rverts = D.rverts; O->rtris = D.rtris; O->meshlets = D.meshlets; O->mpos = D.mpos; O->mbox = D.mbox;
        O->mesh_center[0] = c[0]; O->mesh_center[1] = c[1]; O->mesh_center[2] = c[2]; O->mesh_radius = radius;
    }
    __syncthreads();
    if (threadIdx.x < 8u) D.acc[threadIdx.x] = threadIdx.x < 3u ? 0xFFFFFFFFu : 0u;
}

void zr_launch_vertex_scatter(const XkVertex* src, uint32_t first, uint32_t n, const ZrMeshState& S, hipStream_t s)
{
    if (n == 0) return;
    const size_t words = (size_t)n * 11u;
    hipLaunchKernelGGL(k_vertex_scatter, dim3((uint32_t)((words + 255u) / 256u)), dim3(256), 0, s, (const uint32_t*)src, (uint32_t*)S.raw, first, n, S.n_verts);
}

void zr_launch_mesh_refit(const ZrMeshState& S, uint32_t par, ZrObject* tab, uint32_t n_objs, hipStream_t s)
{
    if (S.n_meshlets) hipLaunchKernelGGL(k_mesh_refit, dim3((S.n_meshlets + ZR_REFIT_WAVES - 1u) / ZR_REFIT_WAVES), dim3(ZR_REFIT_WAVES * WAVE), 0, s, S, par);
    if (S.n_verts) hipLaunchKernelGGL(k_mesh_refit_verts, dim3((S.n_verts + 255u) / 256u), dim3(256), 0, s, S, par);
    hipLaunchKernelGGL(k_table_set_mesh, dim3(1), dim3(64), 0, s, tab, n_objs, S, par);
}
