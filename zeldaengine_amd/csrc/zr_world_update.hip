// zr_world_update.hip — a world applied as a difference (zr_world_update_json): carrying the frame loop's history across a renumbering.
//
// A work item is work_base + instance * n_meshlets + meshlet.  When a world update adds, removes, resizes or reorders objects the kept
// draws get new bases; what the frame loop had learnt about their meshlet-instances - one byte each in the two visibility planes
// (d_visflag: the stamp of the frame that saw it win a pixel) and in the shadow flags (d_sflag: not hidden in the map drawn last) - is
// moved to the new numbers instead of being forgotten.  zr_scene_finalize copies the old planes out first (ranges overlap when a base shifts
// by less than a draw's length, in either direction; a scene that outgrew its pools gets new planes altogether), so k_history_carry is a
// gather from those copies into the live planes: one lane per 4 output bytes, a whole dword at a time where source and destination are
// aligned alike inside one range, byte by byte where they are not.  Bytes no range covers get stamp 0 ("no frame's stamp is 0": not seen,
// tested against Hi-Z in round 2) and shadow flag 1 ("draw in the first launch").
//
// A wrong carry cannot change a pixel - the depth test decides those - only what the rounds cost (tests/test_gpu_world_update.py holds
// the counters of a carried context to an undisturbed twin's).
#include "zr_dev.h"

// the last range whose new_base <= j (ranges sorted by new_base), or -1
__device__ __forceinline__ int history_range_of(const ZrHistoryRange* __restrict__ R, int n, uint32_t j)
{
    int lo = -1, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ld_global(&R[mid].new_base) <= j) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_history_carry(ZrHistoryCarry H)
{
    const uint64_t j64 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (j64 >= H.n_new) return;
    const uint32_t j0 = (uint32_t)j64, nb = min(4u, H.n_new - j0);      // this lane's bytes [j0, j0 + nb)
    uint32_t out0 = 0u, out1 = 0u, out2 = 0x01010101u;
    const int r = history_range_of(H.ranges, (int)H.n_ranges, j0);
    bool whole = false;
    if (r >= 0 && nb == 4u) {
        const uint4 q = ld_global((const uint4*)(H.ranges + r));       // new_base, old_base, count
        const uint32_t off = j0 - q.x, si = q.y + off;
        if (off < q.z && q.z - off >= 4u && (si & 3u) == 0u && (uint64_t)si + 4u <= H.n_old) {
            out0 = ld_global((const uint32_t*)(H.src[0] + si));
            out1 = ld_global((const uint32_t*)(H.src[1] + si));
            out2 = ld_global((const uint32_t*)(H.src[2] + si));
            whole = true;
        }
    }
    if (!whole) {
        // byte by byte: the dword straddles ranges, or source and destination are not aligned alike.  (k walks forward from r: ranges are
        // disjoint and sorted, so a later byte lies in range k, in one that follows it, or in none.)
        int k = r;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            const uint32_t j = j0 + b;
            if (b < nb) {
                while (k + 1 < (int)H.n_ranges && ld_global(&H.ranges[k + 1].new_base) <= j) ++k;
                if (k >= 0) {
                    const uint4 q = ld_global((const uint4*)(H.ranges + k));
                    const uint32_t off = j - q.x, si = q.y + off;
                    if (off < q.z && si < H.n_old) {
                        const uint32_t sh = 8u * b, keep = ~(255u << sh);
                        out0 = (out0 & keep) | (uint32_t)ld_global(H.src[0] + si) << sh;
                        out1 = (out1 & keep) | (uint32_t)ld_global(H.src[1] + si) << sh;
                        out2 = (out2 & keep) | (uint32_t)ld_global(H.src[2] + si) << sh;
                    }
                }
            }
        }
    }
    if (nb == 4u) {
        *(ZR_AS_GLOBAL uint32_t*)(H.dst[0] + j0) = out0;
        *(ZR_AS_GLOBAL uint32_t*)(H.dst[1] + j0) = out1;
        *(ZR_AS_GLOBAL uint32_t*)(H.dst[2] + j0) = out2;
    } else {
        for (uint32_t b = 0; b < nb; ++b) {      // the planes' last bytes (n_new is no multiple of 4)
            *(ZR_AS_GLOBAL uint8_t*)(H.dst[0] + j0 + b) = (uint8_t)(out0 >> (8u * b));
            *(ZR_AS_GLOBAL uint8_t*)(H.dst[1] + j0 + b) = (uint8_t)(out1 >> (8u * b));
            *(ZR_AS_GLOBAL uint8_t*)(H.dst[2] + j0 + b) = (uint8_t)(out2 >> (8u * b));
        }
    }
}

// (a table of no ranges launches nothing: zr_scene_finalize then forgets the history, as it does without a remap)
void zr_launch_history_carry(const ZrHistoryCarry& H, hipStream_t s)
{
    if (H.n_ranges == 0 || H.n_new == 0) return;
    const uint64_t lanes = ((uint64_t)H.n_new + 3u) / 4u;
    hipLaunchKernelGGL(k_history_carry, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, s, H);
}
