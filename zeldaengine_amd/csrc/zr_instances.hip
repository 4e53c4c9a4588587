// zr_instances.hip — instance updates between frames (zr_object_set_instances, zr_object_update_instances_async).
//
// An updated object keeps, on the device: its raw XkInstanceData (what the update calls write), two ZrInstance planes (one per frame
// parity: a frame reads the plane of its parity, through the draw table of its parity) and, per parity, a list of the instances whose
// record in that plane is stale.  k_instance_scatter writes raw values and puts each touched instance on both lists (once: a per-instance
// bit per parity); k_instance_apply rebuilds the listed records of one plane at the head of a frame of that parity.  Both cost what was
// touched, not the instance count.  The ordering between them and the frames lives on the host (zr_instances_host.cpp).
#include "zr_dev.h"

// data[j] replaces instance idx[j] (idx == nullptr: instance first + j); indices >= n_inst are ignored
__global__ void k_instance_scatter(const uint32_t* __restrict__ idx, const XkInstanceData* __restrict__ data, uint32_t first, uint32_t n,
                                   ZrInstanceState S)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = idx ? idx[j] : first + j;
    if (i >= S.n_inst) return;
    S.raw[i] = data[j];
    const uint32_t old = atomicOr(S.dirty + i, 3u);
    if (!(old & 1u)) S.list[0][atomicAdd(S.count + 0, 1u)] = i;
    if (!(old & 2u)) S.list[1][atomicAdd(S.count + 1, 1u)] = i;
}

// plane `par` of the listed instances from their raw values; the grid covers an upper bound of the list's length (known on the host)
__global__ void k_instance_apply(ZrInstanceState S, uint32_t par)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S.count[par]) return;
    const uint32_t i = S.list[par][t];
    S.plane[par][i] = instance_record(S.raw[i]);
    atomicAnd(S.dirty + i, ~(1u << par));
}

// one draw record of a table points at another instance plane
__global__ void k_table_set_inst(ZrObject* __restrict__ tab, uint32_t draw, const ZrInstance* plane)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) tab[draw].inst = plane;
}

void zr_launch_instance_scatter(const uint32_t* idx, const XkInstanceData* data, uint32_t first, uint32_t n, const ZrInstanceState& S, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_instance_scatter, dim3((n + 255u) / 256u), dim3(256), 0, s, idx, data, first, n, S);
}

void zr_launch_instance_apply(const ZrInstanceState& S, uint32_t par, uint32_t bound, hipStream_t s)
{
    if (bound == 0) return;
    hipLaunchKernelGGL(k_instance_apply, dim3((bound + 255u) / 256u), dim3(256), 0, s, S, par);
}

void zr_launch_table_set_inst(ZrObject* tab, uint32_t draw, const ZrInstance* plane, hipStream_t s)
{
    hipLaunchKernelGGL(k_table_set_inst, dim3(1), dim3(64), 0, s, tab, draw, plane);
}
