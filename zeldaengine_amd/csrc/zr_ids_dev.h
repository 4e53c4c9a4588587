// zr_ids_dev.h — winner primitive -> draw -> instance, the device steps the census (zr_ids.hip) and the highlight mask
// (zr_highlight.hip) share.
#pragma once

#include "zr_dev.h"
#include "zr_ids.h"

// the draw that holds primitive p (draws[] is sorted by prim_base; the sentinel is never returned for a scene primitive)
__device__ __forceinline__ uint32_t find_draw(const ZrIdsDraw* __restrict__ draws, uint32_t n, uint32_t p)
{
    uint32_t lo = 0, hi = n - 1u;
    while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if (draws[mid].prim_base <= p) lo = mid; else hi = mid - 1u; }
    return lo;
}

// a pixel's winner is a scene primitive (the sentinel's prim_base is the scene's primitive count; ZR_EMPTY_PRIM is above it)
__device__ __forceinline__ bool ids_scene_prim(const ZrIdsDraw* __restrict__ draws, uint32_t n, uint32_t prim) { return prim < draws[n].prim_base; }

// primitive -> draw for a whole wave, every lane of which calls it; hm = __ballot(hit), not 0.  When every lane's primitive lies in
// the draw of the first lane that has one (the common case), one search for the whole wave; else each lane searches its own.  (A lane
// without a hit gets the first lane's draw.)
__device__ __forceinline__ uint32_t ids_wave_draw(const ZrIdsDraw* __restrict__ draws, uint32_t n, uint32_t prim, bool hit, unsigned long long hm)
{
    const uint32_t p0 = __shfl(prim, __ffsll((long long)hm) - 1);
    uint32_t d = find_draw(draws, n, p0);
    const uint32_t lo0 = draws[d].prim_base, hi0 = draws[d + 1u].prim_base;
    if (__ballot(hit && (prim < lo0 || prim >= hi0)) != 0ull && hit) d = find_draw(draws, n, prim);
    return d;
}

// the primitive's number within its draw (0 for a lane without a hit), and the instance that holds it
__device__ __forceinline__ uint32_t ids_local(const ZrIdsDraw& D, uint32_t prim, bool hit) { return hit ? prim - D.prim_base : 0u; }
__device__ __forceinline__ uint32_t ids_instance(const ZrIdsDraw& D, uint32_t local) { return local / D.n_tris; }
