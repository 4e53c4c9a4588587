// zr_instances.hip — instance updates between frames (zr_object_set_instances, zr_object_update_instances_async) and visibility
// (zr_object_set_instance_visibility, zr_object_update_instance_visibility_async, zr_object_set_visible).
//
// An updated object keeps, on the device: its raw XkInstanceData and a visibility byte per instance (what the update calls write), two
// ZrInstance planes (one per frame parity: a frame reads the plane of its parity, through the draw table of its parity) and, per parity, a
// list of the instances whose record in that plane is stale.  k_instance_scatter / k_visibility_scatter write raw values / bytes and put
// each touched instance on both lists (once: a per-instance bit per parity, so an instance moved AND hidden is listed once);
// k_instance_apply rebuilds the listed records of one plane - transform and hidden word - at the head of a frame of that parity.  All cost
// what was touched, not the instance count.  The ordering between them and the frames lives on the host (zr_instances_host.cpp).
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

// visible[j] != 0 shows, == 0 hides instance idx[j] (idx == nullptr: instance first + j); indices >= n_inst are ignored
__global__ void k_visibility_scatter(const uint32_t* __restrict__ idx, const uint8_t* __restrict__ visible, uint32_t first, uint32_t n,
                                     ZrInstanceState S)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = idx ? idx[j] : first + j;
    if (i >= S.n_inst) return;
    S.vis[i] = visible[j] ? 1u : 0u;
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
    ZrInstance I = instance_record(S.raw[i]);
    I._pad[0] = S.vis[i] ? 0.0f : 1.0f;      // (the culls test the word's bits: 0 = shown)
    S.plane[par][i] = I;
    atomicAnd(S.dirty + i, ~(1u << par));
}

// one draw record of a table points at another instance plane
__global__ void k_table_set_inst(ZrObject* __restrict__ tab, uint32_t draw, const ZrInstance* plane)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) tab[draw].inst = plane;
}

// one draw record of a table is hidden / shown as a whole (ZR_OBJ_HIDDEN; the record's other flags stay)
__global__ void k_table_set_hidden(ZrObject* __restrict__ tab, uint32_t draw, uint32_t hidden)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) tab[draw].flags = (tab[draw].flags & ~ZR_OBJ_HIDDEN) | (hidden ? ZR_OBJ_HIDDEN : 0u);
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

void zr_launch_visibility_scatter(const uint32_t* idx, const uint8_t* visible, uint32_t first, uint32_t n, const ZrInstanceState& S, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_visibility_scatter, dim3((n + 255u) / 256u), dim3(256), 0, s, idx, visible, first, n, S);
}

void zr_launch_table_set_hidden(ZrObject* tab, uint32_t draw, uint32_t hidden, hipStream_t s)
{
    hipLaunchKernelGGL(k_table_set_hidden, dim3(1), dim3(64), 0, s, tab, draw, hidden);
}
