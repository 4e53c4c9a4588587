// zr_raycast.hip — k_raycast: the nearest hit of each ray in the scene as the frame enqueued last drew it (zelda_render.h, "casting rays";
// the rule is zr_raycast.h's, DESIGN.md section 5, "Casting rays", has the levels and the margin's derivation).
//
// One workgroup of 256 threads (four waves) per ray, three levels, every compaction a ballot and one LDS atomic per wave:
//   1 instances   all lanes sweep the instances of the scene's draws (a non-instanced draw is one instance), 256 a step: hidden ones
//                 dropped, the whole-mesh sphere - through the instance record and M - against the ray's segment; survivors go to an LDS
//                 list, which is drained whenever another step might not fit (a ray down a row of any number of instances works)
//   2 meshlets    a wave per listed instance, lanes over its meshlets: the meshlet's sphere the same way; survivors go to a second list,
//                 drained the same way
//   3 triangles   a wave per listed meshlet: lanes below VertexCount stage the corners' sheared coordinates in LDS once, the lanes
//                 then take the triangles (two rounds above 64) and apply the rule; the wave's least 64-bit key (t ordered | global
//                 primitive id) is reduced on the DPP network and merged into the workgroup's with one LDS 64-bit min
// The winner's corner words are fetched again by one thread, which tests it once more (the same arithmetic, the same t) for u, v, the
// facing and the normal, and stores the record.  A record whose R is no rotation gets no sphere test and is kept, as in the culls.
// Every loop bound is an integer count of the draw table; NaN / infinite records end in comparisons that are false: kept, then missed.
// No running-best pruning: a sphere is tested against the whole segment (see DESIGN.md for what it would take).
#include "zr_dev.h"
#include "zr_ids.h"
#include "zr_raycast.h"

#define RC_THREADS 256u
#define RC_WAVES (RC_THREADS / WAVE)
#define RC_ICAP 512u                  // listed instances; a step appends at most RC_THREADS
#define RC_MCAP 512u                  // listed meshlets; a step appends at most RC_THREADS
// The absolute part of a sphere's margin, in units of (|centre - o|_1 + r + |t_c| |d|_1): 64 u, u = 2^-24 (the rule's own
// error is below 16 u of it, this test's below 8 u)
#define RC_EPS 3.814697265625e-6f

struct RcShared {
    uint4 ilist[RC_ICAP];             // draw, instance, the draw's meshlet count, 0
    uint4 mlist[RC_MCAP];             // draw, instance, meshlet, 0
    float corner[RC_WAVES][WAVE][3];  // a wave's meshlet: its vertices in the ray's sheared coordinates
    unsigned long long best;
    uint32_t icount, mcount, any;
};

__device__ __forceinline__ void rc_append(bool keep, uint4 e, uint4* list, uint32_t* count)
{
    const unsigned long long m = __ballot(keep);
    if (m == 0ull) return;
    const uint32_t lane = threadIdx.x & 63u, first = (uint32_t)__builtin_ctzll(m);
    uint32_t base = 0u;
    if (lane == first) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)first);
    if (keep) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = e;
}

// Can the rule accept a triangle inside the sphere (centre co ahead of M, radius r there)?  false only when it cannot: the distance from
// the centre to the segment [t_min, t_max] exceeds the inflated radius.  Every doubt - a NaN, an overflow - compares false and keeps.
struct RcRayBound { float dd, d1; bool ok; };
__device__ __forceinline__ RcRayBound rc_ray_bound(const ZrRcRay& R)
{
    RcRayBound B;
    B.dd = zr_dot(zr3(R.d[0], R.d[1], R.d[2]), zr3(R.d[0], R.d[1], R.d[2]));
    B.d1 = __builtin_fabsf(R.d[0]) + __builtin_fabsf(R.d[1]) + __builtin_fabsf(R.d[2]);
    B.ok = B.dd >= 1e-30f && B.dd <= 1e30f;       // (outside it the quotient below says nothing: no sphere rejects)
    return B;
}
__device__ __forceinline__ bool rc_sphere_reaches(const ZrRcRay& R, const RcRayBound& B, const float* M, float m_scale, zf3 co, float r)
{
    if (!B.ok) return true;
    const zf4 c4 = zr_mat4_point(M, co);
    const zf3 d = zr3(R.d[0], R.d[1], R.d[2]);
    const zf3 oc = zr3(c4.x - R.o[0], c4.y - R.o[1], c4.z - R.o[2]);
    const float tc = __builtin_fminf(__builtin_fmaxf(zr_dot(oc, d) / B.dd, R.t_min), R.t_max);
    const zf3 q = zr3(__builtin_fmaf(-tc, d.x, oc.x), __builtin_fmaf(-tc, d.y, oc.y), __builtin_fmaf(-tc, d.z, oc.z));
    const float rw = r * m_scale;
    float reach = __builtin_fmaf(rw, 1.001f, 1e-5f * (__builtin_fabsf(c4.x) + __builtin_fabsf(c4.y) + __builtin_fabsf(c4.z) + 1.0f));      // (the culls' margin)
    reach += RC_EPS * (__builtin_fabsf(oc.x) + __builtin_fabsf(oc.y) + __builtin_fabsf(oc.z) + rw + __builtin_fabsf(tc) * B.d1);
    return !(zr_dot(q, q) > reach * reach * 1.000001f);
}

__device__ __forceinline__ uint32_t wave_umin(uint32_t v) { return (uint32_t)wave_min((int)(v ^ 0x80000000u)) ^ 0x80000000u; }

// A corner's world position: the xyz of zr_mat4_point(M, vs_position(p, I, instanced)), the camera pass's own arithmetic
__device__ __forceinline__ void rc_world_corner(const ZrRayArgs& A, const ZrObject* __restrict__ O, uint32_t v, const ZrInstance& I, bool instanced, float* P)
{
    const float4 pp = ld_global(O->mpos + v);
    const zf4 w = zr_mat4_point(A.M, vs_position(zr3(pp.x, pp.y, pp.z), I, instanced));
    P[0] = w.x; P[1] = w.y; P[2] = w.z;
}

// Level 3: the calling wave against one listed meshlet
__device__ __forceinline__ void rc_meshlet(const ZrRayArgs& A, const ZrRcRay& R, RcShared& S, uint4 e, uint32_t wave, uint32_t lane)
{
    const ZrObject* __restrict__ O = A.objs + e.x;
    const XkMeshlet* __restrict__ ml = O->meshlets + e.z;
    const uint4 mh = ld_global((const uint4*)ml);            // VertexOffset, VertexCount, TriangleOffset, TriangleCount
    const uint32_t tri_base = ld_global(&ml->BindlessContext);
    const uint32_t vcount = min(mh.y, (uint32_t)WAVE), tcount = min(mh.w, 2u * WAVE);
    const bool instanced = O->instanced != 0u;
    const ZrInstance I = ld_record(O->inst + e.y);
    const uint32_t pbase = O->prim_base + e.y * O->n_tris;
    const uint2* __restrict__ tw = O->mtri + tri_base;
    lds_fence();                                             // this wave's previous readers are done with its corners
    if (lane < vcount) {
        float P[3];
        rc_world_corner(A, O, mh.x + lane, I, instanced, P);
        const ZrRcCorner c = zr_rc_corner(R, P);
        S.corner[wave][lane][0] = c.x; S.corner[wave][lane][1] = c.y; S.corner[wave][lane][2] = c.z;
    }
    lds_fence();
    unsigned long long key = ZR_RAY_NO_KEY;
#pragma unroll
    for (uint32_t round = 0; round < 2u; ++round) {
        const uint32_t ti = lane + round * WAVE;
        if (ti >= tcount) continue;
        const uint2 w = ld_global(tw + ti);
        const uint32_t i0 = w.x & 255u, i1 = (w.x >> 8) & 255u, i2 = (w.x >> 16) & 255u;
        if (i0 >= vcount || i1 >= vcount || i2 >= vcount) continue;
        ZrRcCorner a, b, c;
        a.x = S.corner[wave][i0][0]; a.y = S.corner[wave][i0][1]; a.z = S.corner[wave][i0][2];
        b.x = S.corner[wave][i1][0]; b.y = S.corner[wave][i1][1]; b.z = S.corner[wave][i1][2];
        c.x = S.corner[wave][i2][0]; c.y = S.corner[wave][i2][1]; c.z = S.corner[wave][i2][2];
        const ZrRcTri T = zr_rc_triangle(R, a, b, c);
        if (!T.hit || ((A.flags & ZR_RAY_CULL_BACK) && T.back)) continue;
        const unsigned long long k = zr_rc_key(T.t, pbase + w.y);
        key = k < key ? k : key;
    }
    const uint32_t hi = (uint32_t)(key >> 32), mhi = wave_umin(hi);
    const uint32_t mlo = wave_umin(hi == mhi ? (uint32_t)key : 0xFFFFFFFFu);
    const unsigned long long wkey = (unsigned long long)mhi << 32 | mlo;
    if (lane == 0u && wkey != ZR_RAY_NO_KEY) { atomicMin(&S.best, wkey); S.any = 1u; }
}

// The list of meshlets drained: a wave per entry.  (Every thread of the workgroup calls it; ends with the list empty.)
__device__ __forceinline__ void rc_drain_meshlets(const ZrRayArgs& A, const ZrRcRay& R, RcShared& S, uint32_t wave, uint32_t lane)
{
    __syncthreads();
    const uint32_t n = min(S.mcount, RC_MCAP);
    for (uint32_t k = wave; k < n; k += RC_WAVES) rc_meshlet(A, R, S, S.mlist[k], wave, lane);
    __syncthreads();
    if (threadIdx.x == 0u) S.mcount = 0u;
    __syncthreads();
}

// The list of instances drained: a wave per entry, its lanes over the draw's meshlets.  Ends with both lists empty.
__device__ __forceinline__ void rc_drain_instances(const ZrRayArgs& A, const ZrRcRay& R, const RcRayBound& B, RcShared& S, uint32_t wave, uint32_t lane)
{
    __syncthreads();
    const uint32_t n = min(S.icount, RC_ICAP);
    const bool bounds = !(A.flags & ZR_RAY_NO_BOUNDS);
    for (uint32_t e0 = 0; e0 < n; e0 += RC_WAVES) {
        uint32_t nm_max = 0u;
        for (uint32_t k = 0; k < RC_WAVES; ++k) if (e0 + k < n) nm_max = max(nm_max, S.ilist[e0 + k].z);
        const bool mine = e0 + wave < n;
        const uint4 e = mine ? S.ilist[e0 + wave] : make_uint4(0u, 0u, 0u, 0u);
        const ZrObject* __restrict__ O = A.objs + e.x;
        const bool instanced = mine && O->instanced != 0u;
        ZrInstance I = {};
        if (mine) I = ld_record(O->inst + e.y);
        const bool test = bounds && (!instanced || is_rotation(I.R));
        for (uint32_t m0 = 0; m0 < nm_max; m0 += WAVE) {
            __syncthreads();
            const uint32_t listed = S.mcount;
            __syncthreads();
            if (listed + RC_THREADS > RC_MCAP) {
                rc_drain_meshlets(A, R, S, wave, lane);
                if ((A.flags & ZR_RAY_ANY_HIT) && S.any) break;
            }
            const uint32_t m = m0 + lane;
            bool keep = mine && m < e.z;
            if (keep && test) {
                const float4 bs = ld_global((const float4*)(O->meshlets + m) + 1);      // centre.xyz radius
                keep = rc_sphere_reaches(R, B, A.M, A.m_scale, vs_position(zr3(bs.x, bs.y, bs.z), I, instanced), bs.w * (instanced ? __builtin_fabsf(I.s) : 1.0f));
            }
            rc_append(keep, make_uint4(e.x, e.y, m, 0u), S.mlist, &S.mcount);
        }
        __syncthreads();
        if ((A.flags & ZR_RAY_ANY_HIT) && S.any) break;
    }
    rc_drain_meshlets(A, R, S, wave, lane);
    if (threadIdx.x == 0u) S.icount = 0u;
    __syncthreads();
}

// The winner's record: its draw, instance and triangle from the primitive id, its corner words from its meshlet's list
__device__ __forceinline__ zr_ray_hit rc_winner(const ZrRayArgs& A, const ZrRcRay& R, uint32_t prim)
{
    const int d = find_object_prim(A.objs, (int)A.n_draws, prim);
    const ZrObject* __restrict__ O = A.objs + d;
    const uint32_t nt = O->n_tris, local = prim - O->prim_base;
    if (nt == 0u) return zr_rc_miss(0u);
    const uint32_t inst = local / nt, tri = local - inst * nt;
    const XkMeshlet* __restrict__ ml = O->meshlets + ld_global(O->tri_meshlet + tri);
    const uint4 mh = ld_global((const uint4*)ml);
    const uint2* __restrict__ tw = O->mtri + ld_global(&ml->BindlessContext);
    const uint32_t tcount = min(mh.w, 2u * WAVE);
    uint32_t word = 0u; bool found = false;
    for (uint32_t k = 0; k < tcount; ++k) { const uint2 w = ld_global(tw + k); if (w.y == tri) { word = w.x; found = true; } }
    if (!found) return zr_rc_miss(0u);
    const ZrInstance I = ld_record(O->inst + inst);
    const bool instanced = O->instanced != 0u;
    float Pa[3], Pb[3], Pc[3];
    rc_world_corner(A, O, mh.x + (word & 255u), I, instanced, Pa);
    rc_world_corner(A, O, mh.x + ((word >> 8) & 255u), I, instanced, Pb);
    rc_world_corner(A, O, mh.x + ((word >> 16) & 255u), I, instanced, Pc);
    return zr_rc_record(R, Pa, Pb, Pc, A.draws[d].object, inst, tri);
}

__global__ __launch_bounds__(RC_THREADS) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_raycast(ZrRayArgs A)
{
    __shared__ RcShared S;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const zr_ray ray = ld_record(A.rays + blockIdx.x);
    const ZrRcRay R = zr_rc_ray(ray);
    zr_ray_hit out = zr_rc_miss(R.valid ? 0u : ZR_RAY_INVALID);
    if (R.valid) {                                           // (the same for every thread of the workgroup)
        if (threadIdx.x == 0u) { S.best = ZR_RAY_NO_KEY; S.icount = 0u; S.mcount = 0u; S.any = 0u; }
        __syncthreads();
        const RcRayBound B = rc_ray_bound(R);
        const bool bounds = !(A.flags & ZR_RAY_NO_BOUNDS);
        for (uint32_t base = 0; base < A.n_inst; base += RC_THREADS) {
            __syncthreads();
            const uint32_t listed = S.icount;
            __syncthreads();
            if (listed + RC_THREADS > RC_ICAP) {
                rc_drain_instances(A, R, B, S, wave, lane);
                if ((A.flags & ZR_RAY_ANY_HIT) && S.any) break;
            }
            const uint32_t g = base + threadIdx.x;
            bool keep = false;
            uint4 e = make_uint4(0u, 0u, 0u, 0u);
            if (g < A.n_inst) {
                int lo = 0, hi = (int)A.n_draws - 1;         // the draw of instance g
                while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (A.objs[mid].inst_base <= g) lo = mid; else hi = mid - 1; }
                const ZrObject* __restrict__ O = A.objs + lo;
                const uint32_t inst = g - O->inst_base;
                const bool instanced = O->instanced != 0u;
                if (inst < O->n_inst && !(O->flags & (ZR_OBJ_HIDDEN | ZR_OBJ_SKY)) && O->n_meshlets != 0u) {
                    const ZrInstance I = ld_record(O->inst + inst);
                    keep = zr_f2u(I._pad[0]) == 0u;
                    if (keep && bounds && (!instanced || is_rotation(I.R)))
                        keep = rc_sphere_reaches(R, B, A.M, A.m_scale, vs_position(zr3(O->mesh_center[0], O->mesh_center[1], O->mesh_center[2]), I, instanced),
                                                 O->mesh_radius * (instanced ? __builtin_fabsf(I.s) : 1.0f));
                    e = make_uint4((uint32_t)lo, inst, O->n_meshlets, 0u);
                }
            }
            rc_append(keep, e, S.ilist, &S.icount);
        }
        if (!((A.flags & ZR_RAY_ANY_HIT) && S.any)) rc_drain_instances(A, R, B, S, wave, lane);
        __syncthreads();
        if (threadIdx.x == 0u) {
            const unsigned long long best = S.best;
            if (A.flags & ZR_RAY_ANY_HIT) out = zr_rc_miss(S.any ? ZR_RAY_HIT : 0u);
            else if (best != ZR_RAY_NO_KEY) out = rc_winner(A, R, (uint32_t)best);
        }
    }
    if (threadIdx.x == 0u) {                                 // 48 bytes, three 16-byte stores
        uint4* __restrict__ dst = reinterpret_cast<uint4*>(A.hits + blockIdx.x);
        dst[0] = make_uint4(out.object, out.instance, out.triangle, out.flags);
        dst[1] = make_uint4(zr_f2u(out.t), zr_f2u(out.u), zr_f2u(out.v), out.reserved);
        dst[2] = make_uint4(zr_f2u(out.normal[0]), zr_f2u(out.normal[1]), zr_f2u(out.normal[2]), out.reserved2);
    }
}

void zr_launch_raycast(const ZrRayArgs& A, hipStream_t s)
{
    if (A.n_rays == 0u) return;
    hipLaunchKernelGGL(k_raycast, dim3(A.n_rays), dim3(RC_THREADS), 0, s, A);
}
