// zr_ids.hip — object identity of the last frame: a census of the winner plane the resolve keeps while id capture is on
// (zr_set_id_capture).  k_id_census maps every pixel of a rectangle to its (object, instance) slot and counts, per slot, the pixels it
// won and (picking) its nearest pixel; k_id_hits turns the slots a pick touched into zr_hit records and clears them again.
// Integer atomics only: every result is independent of arrival order, bit for bit.
#include "zr_ids_dev.h"      // find_draw, the wave's one-search shortcut, primitive -> instance: shared with zr_highlight.hip

// One lane per pixel of the rectangle, row-major: a wave reads 64 consecutive pixels of a row (256 B of the plane).
// Per wave, the lanes that share a slot are aggregated before any atomic (one add, and one 64-bit min when picking, per distinct slot):
// instances cover runs of pixels, so a wave usually holds 1-3 slots.
template <int MODE>
__global__ __launch_bounds__(256) void k_id_census(ZrIdsArgs A)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool in = i < A.w * A.h;
    uint32_t p = 0u, prim = ZR_EMPTY_PRIM;
    if (in) {
        const uint32_t ry = i / A.w, rx = i - ry * A.w;
        p = (A.y0 + ry) * A.W + A.x0 + rx;
        prim = A.prim[p];
    }
    const bool hit = ids_scene_prim(A.draws, A.n_draws, prim);
    const unsigned long long hm = __ballot(hit);
    if (hm == 0ull) {          // (wave-uniform)
        if (MODE == ZR_IDS_OBJECTS && in) A.obj_plane[p] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        return;
    }
    const ZrIdsDraw D = A.draws[ids_wave_draw(A.draws, A.n_draws, prim, hit, hm)];
    const uint32_t inst = ids_instance(D, ids_local(D, prim, hit));
    if (MODE == ZR_IDS_OBJECTS) {
        if (in) A.obj_plane[p] = hit ? make_uint2(D.object, inst) : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        return;
    }
    const uint32_t slot = D.slot_base + inst;
    unsigned long long key = ~0ull;
    if (MODE == ZR_IDS_PICK && hit) key = (unsigned long long)__float_as_uint(A.depth[p]) << 32 | p;   // depth >= 0: bit order = value order
    const int lane = (int)__lane_id();
    unsigned long long rem = hm;
    while (rem) {              // (wave-uniform: one round per distinct slot of the wave)
        const int leader = __ffsll((long long)rem) - 1;
        const uint32_t ls = __shfl(slot, leader);
        const bool mine = hit && slot == ls;
        const unsigned long long same = __ballot(mine);
        unsigned long long kmin = mine ? key : ~0ull;
        if (MODE == ZR_IDS_PICK)
            for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_xor(kmin, o); kmin = u < kmin ? u : kmin; }
        if (lane == leader) {
            const uint32_t old = atomicAdd(&A.counts[ls], (uint32_t)__popcll(same));
            if (MODE == ZR_IDS_PICK) {
                atomicMin(&A.keys[ls], kmin);
                if (old == 0u) A.hit_list[atomicAdd(A.n_hits, 1u)] = ls;      // the first wave to touch the slot lists it
            }
        }
        rem &= ~same;
    }
}

__global__ __launch_bounds__(256) void k_id_hits(ZrIdsArgs A, uint32_t n, zr_hit* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = A.hit_list[i];
    const unsigned long long key = A.keys[s];
    const uint32_t p = (uint32_t)key, prim = A.prim[p];
    const ZrIdsDraw D = A.draws[find_draw(A.draws, A.n_draws, prim)];
    const uint32_t local = ids_local(D, prim, true), inst = ids_instance(D, local);
    zr_hit h;
    h.object = D.object; h.instance = inst; h.pixels = A.counts[s]; h.triangle = local - inst * D.n_tris;
    h.y = p / A.W; h.x = p - h.y * A.W; h.depth = __uint_as_float((uint32_t)(key >> 32)); h.reserved = 0u;
    out[i] = h;
    A.counts[s] = 0u; A.keys[s] = ~0ull;
}

// ------------------------------------------------------------------------------------------------ launchers (C++ linkage, used by zr_readback.cpp)

void zr_launch_id_census(const ZrIdsArgs& A, int mode, hipStream_t s)
{
    const uint32_t n = A.w * A.h;
    if (n == 0u) return;
    const dim3 grid((n + 255u) / 256u), block(256);
    if (mode == ZR_IDS_PICK) hipLaunchKernelGGL(k_id_census<ZR_IDS_PICK>, grid, block, 0, s, A);
    else if (mode == ZR_IDS_OBJECTS) hipLaunchKernelGGL(k_id_census<ZR_IDS_OBJECTS>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(k_id_census<ZR_IDS_COVERAGE>, grid, block, 0, s, A);
}

void zr_launch_id_hits(const ZrIdsArgs& A, uint32_t n, zr_hit* out, hipStream_t s)
{
    if (n == 0u) return;
    hipLaunchKernelGGL(k_id_hits, dim3((n + 255u) / 256u), dim3(256), 0, s, A, n, out);
}
