// zr_shadow.hip — the shadow pass (ZE:3239-3393) as meshlet-level binning: k_bin_count / k_scan / k_bin_fill (per-tile lists of
// self-contained 32-byte meshlet records), k_raster_chunks<LATE> (persistent workgroups, a 44 x 44 key window in LDS), k_shadow_slow (the
// triangles it left to the clipper), k_shadow_occlusion (the map as a running minimum hides casters), k_count_shadow.  See zr_dev.h for
// the map of the kernel files.
#include "zr_dev.h"
#include "zr_raster.h"

// Per-tile entry counts from the rects.  Counting goes through an LDS histogram per 1024 work items so that a hot
// tile costs one global atomic per workgroup instead of one per meshlet-instance (same-address atomics serialise).
// (Ownership of the map's tiles was decided per meshlet by k_cull_box: an accepted meshlet is listed in every tile of its rect.)
// Z.phase 1 (occlusion culling, see k_shadow_occlusion): only the meshlet-instances flagged last frame are listed.
__global__ __launch_bounds__(1024) void k_bin_count(ZrPass P, const uint32_t* __restrict__ work, const uint32_t* __restrict__ rects,
                                                    uint32_t* __restrict__ tile_count, ZrHiz Z, const ZrDevStats* __restrict__ stats)
{
    extern __shared__ uint32_t hist[];
    const uint32_t n_tiles = P.tiles_x * P.tiles_y;
    const uint32_t n_vis = P.use_worklist ? stats->n_vis_work[0] : P.n_work;
    if (blockIdx.x * 1024u >= n_vis) return;            // the grid is sized for every meshlet-instance of the scene
    hist_clear(hist, n_tiles);
    __syncthreads();
    const uint32_t w = blockIdx.x * 1024u + threadIdx.x;
    if (w < n_vis) {
        uint32_t r = rects[w];
        if (r != ZR_RECT_CULLED && Z.phase && Z.vis_prev[P.use_worklist ? work[w] : w] != (uint8_t)Z.vis_stamp) r = ZR_RECT_CULLED;
        if (r != ZR_RECT_CULLED) hist_add_rect(hist, rect_unpack(r), P.tiles_x);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_tiles; i += 1024u) { const uint32_t c = hist[i]; if (c) atomicAdd(&tile_count[i], c); }
}

// Exclusive scan of tile_count[0..n) into tile_offset[0..n] and of the per-tile work-unit counts ceil(count / chunk)
// into chunk_offset[0..n]; lays out the rasteriser's work units (tile, first entry, end, kind); zeroes tile_count and tile_cursor
// for the fill and resets the work counter.
__global__ __launch_bounds__(1024) void k_scan(uint32_t* __restrict__ tile_count, uint32_t* __restrict__ tile_offset,
                                               uint32_t* __restrict__ tile_cursor, uint32_t* __restrict__ chunk_offset,
                                               uint4* __restrict__ chunk_tab, uint32_t chunk_cap,
                                               uint32_t n, uint32_t capacity, ZrDevStats* __restrict__ stats, uint32_t chunk)
{
    __shared__ uint32_t part[1024];
    __shared__ uint32_t cpart[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t b = tid * per, e = min(n, b + per);
    uint32_t s = 0, cs = 0;
    for (uint32_t i = b; i < e; ++i) s += tile_count[i];
    part[tid] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint32_t v = (tid >= off) ? part[tid - off] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    for (uint32_t i = b; i < e; ++i) cs += (tile_count[i] + chunk - 1u) / chunk;
    cpart[tid] = cs;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint32_t cv = (tid >= off) ? cpart[tid - off] : 0u;
        __syncthreads();
        cpart[tid] += cv;
        __syncthreads();
    }
    uint32_t run = part[tid] - s, crun = cpart[tid] - cs;
    for (uint32_t i = b; i < e; ++i) {
        const uint32_t c = tile_count[i];
        tile_offset[i] = run;
        chunk_offset[i] = crun;
        // one record per raster work unit: (tile, first entry, end, kind): the rasteriser finds its unit with one load, not a search
        const uint32_t nu = (c + chunk - 1u) / chunk;
        for (uint32_t k = 0; k < nu; ++k)
            if (crun + k < chunk_cap) chunk_tab[crun + k] = make_uint4(i, run + k * chunk, run + min(c, (k + 1u) * chunk), 0u);
        run += c; crun += nu;
        tile_count[i] = 0; tile_cursor[i] = 0;
    }
    if (tid < 32u) stats->covered_part[tid] = 0;      // k_shadow_occlusion's tally (32 partial sums)
    if (tid == 1023) {
        tile_offset[n] = part[1023];
        chunk_offset[n] = cpart[1023];
        stats->bin_entries[0] = part[1023];
        stats->n_chunks[0] = min(cpart[1023], chunk_cap);
        stats->chunk_counter[0] = 0;
        // what the kernels after this one accumulate for the pass starts from zero here: the shadow pipeline's block is not touched by
        // k_frame_begin (the pipeline does not wait for the camera lane)
        stats->survivors[0] = 0; stats->n_slow[0] = 0;
        stats->overflow = part[1023] > capacity ? 1u : 0u;
        stats->n_chunks[1] = 0; stats->chunk_counter[1] = 0; stats->shadow_late = 0;      // (k_shadow_occlusion's late units)
        if (part[1023] > capacity) stats->overflow_sticky = ZR_OVF_BINS;
    }
}

// Scatter meshlet-instance ids into the per-tile lists.  Same LDS aggregation as k_bin_count: the workgroup reserves
// a contiguous range per tile with one global atomic, then hands out slots from LDS.
__global__ __launch_bounds__(1024) void k_bin_fill(ZrPass P, const ZrObject* __restrict__ objs, const uint32_t* __restrict__ work,
                                                   const uint32_t* __restrict__ rects,
                                                   const uint32_t* __restrict__ tile_offset, uint32_t* __restrict__ tile_cursor,
                                                   ZrBinEntry* __restrict__ bins, ZrHiz Z, ZrDevStats* __restrict__ stats)
{
    extern __shared__ uint32_t hist[];
    __shared__ uint32_t tot;
    const uint32_t n_tiles = P.tiles_x * P.tiles_y;
    const uint32_t n_vis = P.use_worklist ? stats->n_vis_work[0] : P.n_work;
    if (blockIdx.x * 1024u >= n_vis) return;
    hist_clear(hist, n_tiles);
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    const uint32_t k = blockIdx.x * 1024u + threadIdx.x;
    uint32_t r = ZR_RECT_CULLED, w = 0;
    if (k < n_vis) {
        r = rects[k]; w = P.use_worklist ? work[k] : k;
        if (r != ZR_RECT_CULLED && Z.phase && Z.vis_prev[w] != (uint8_t)Z.vis_stamp) r = ZR_RECT_CULLED;      // (as in k_bin_count)
    }
    const TileRect R = rect_unpack(r);
    if (r != ZR_RECT_CULLED) hist_add_rect(hist, R, P.tiles_x);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_tiles; i += 1024u) {
        const uint32_t c = hist[i];
        if (c) hist[i] = tile_offset[i] + atomicAdd(&tile_cursor[i], c);      // hist now holds the next free slot
    }
    __syncthreads();
    if (r != ZR_RECT_CULLED) {
        // decode the work id once; every tile of the rect gets the same self-contained record
        const ZrBinEntry be = bin_entry(objs, (int)P.n_objects, w);
        for (uint32_t ty = R.ty0; ty <= R.ty1; ++ty)
            for (uint32_t tx = R.tx0; tx <= R.tx1; ++tx) {
                const uint32_t pos = atomicAdd(&hist[ty * P.tiles_x + tx], 1u);
                if (pos < P.bin_capacity) bins[pos] = be;
            }
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(r != ZR_RECT_CULLED));
    if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(&tot, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && tot) atomicAdd(&stats->survivors[0], tot);
}

// The shadow rasteriser's per-wave ring of surviving triangles, SoA in LDS: 3 x (tile-relative X | Y << 16, z) + prim, QCAP words apart.
// This lane's entry, at q, drawn into the window's keys:
__device__ __forceinline__ void queue_draw(const int* q, const TileCtx& T, uint32_t* keys32)
{
    const RecTri t = tri_unpack((uint32_t)q[0 * QCAP], (uint32_t)q[1 * QCAP], (uint32_t)q[2 * QCAP], (uint32_t)q[3 * QCAP], (uint32_t)q[4 * QCAP],
                                (uint32_t)q[5 * QCAP], (uint32_t)q[6 * QCAP]);
    raster_sub<ZR_MODE_SHADOW, true>(t.a, t.b, t.c, t.prim, T, nullptr, keys32);
}

// Persistent chunk rasteriser.  A chunk = up to ZR_CHUNK consecutive entries of ONE tile's bin list, so a hot tile is
// spread over many workgroups and the pass is bounded by total work, not by the fullest tile.  Every workgroup pulls
// chunk ids from one device counter until they run out (each wave reaches the exit test).  Per chunk: clear the
// window's LDS keys, 4 waves rasterise the chunk's meshlets into them (ds_min), then the touched keys are merged into
// the shadow map in HBM (float bits as uint) with global atomic min: the merge IS the LESS_OR_EQUAL depth write.
// Triangles that need the clipper (or the 64-bit walk) are not rasterised here but appended, with their tile, to `slow` for
// k_shadow_slow: without the call to raster_clipped in its loop the kernel needs half the registers, i.e. twice the waves per SIMD
// fit - next to each other and next to the other lane's kernels.
// LATE (after k_shadow_occlusion): unit u is the ONE entry bins[bin_capacity - 1 - u], its tile in the record's prim_base
// (the shadow pass has no use for a primitive id); the units are counted in slot 1 of the pipeline's block, slow triangles stay in slot 0.
template <bool LATE>
__global__ __launch_bounds__(RTHREADS) __attribute__((amdgpu_waves_per_eu(ZR_RASTER_WAVES_DEFER)))
void k_raster_chunks(ZrPass P, const ZrObject* __restrict__ objs, const uint4* __restrict__ chunk_tab,
                     const ZrBinEntry* __restrict__ bins, ZrDevStats* __restrict__ stats,
                     uint32_t* __restrict__ shadow_bits, uint4* __restrict__ slow, uint32_t slow_cap)
{
    __shared__ uint32_t keys32[SPAN_PIX(ZR_MODE_SHADOW)];      // the key window
    __shared__ int4 vstage[RW][WAVE];
    // per-wave ring of surviving triangles (queue_draw).  Only small triangles (edges under 64 px) that reach the tile are queued, so a
    // relative coordinate lies within [-16384, 24576] sub-pixel units and fits 16 bits.
    __shared__ int queue[RW][7][QCAP];
    __shared__ uint32_t cur_chunk;

    // the wave index is made KNOWN-uniform: entry indices, bin records, the instance record and every pointer derived from them
    // then live in SGPRs and are fetched with scalar loads - some 30 VGPRs less in the hot loop (one more wave per SIMD, and this
    // kernel waits on dependent loads most of the time)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = wave_uniform(tid >> 6);
    const uint32_t n_chunks = LATE ? min(stats->n_chunks[1], P.bin_capacity - min(stats->bin_entries[0], P.bin_capacity)) : stats->n_chunks[0];

    uint32_t chunk = blockIdx.x;
    bool first = true;
    for (;;) {
        if (chunk >= n_chunks) break;
        keys_clear(keys32, tid, RTHREADS);
        __syncthreads();
        // this work unit: (tile, first entry, end) as k_scan laid it out: one load, not a search over the tiles' chunk offsets
        uint4 ct;
        if (LATE) { const uint32_t idx = P.bin_capacity - 1u - chunk; ct = make_uint4(((const uint4*)bins)[2u * idx + 1u].w, idx, idx + 1u, 0u); }
        else ct = chunk_tab[chunk];
        const uint32_t tile = ct.x, beg = ct.y, end = min(ct.z, P.bin_capacity);
        int tpx0, tpy0;
        const TileCtx T = tile_ctx(P, tile, tpx0, tpy0);
        const int ox = tpx0 * 256, oy = tpy0 * 256;

        uint32_t qhead = 0, qn = 0;
        // The next entry's 32-byte record is fetched (vector loads, vmcnt-ordered) while the current one is processed; every
        // load of a meshlet then depends on that record alone.
        const uint4* __restrict__ rec = (const uint4*)bins;
        uint4 n0 = make_uint4(0, 0, 0, 0), n1 = n0;
        if (beg + wv < end) { n0 = rec[2u * (beg + wv)]; n1 = rec[2u * (beg + wv) + 1u]; }
        for (uint32_t e = beg + wv; e < end; e += RW) {
            const uint4 r0 = n0, r1 = n1;
            if (e + RW < end) { n0 = rec[2u * (e + RW)]; n1 = rec[2u * (e + RW) + 1u]; }
            const ZrBinEntry be = { (const float4*)(((unsigned long long)wave_uniform(r0.y) << 32) | wave_uniform(r0.x)),
                                    (const uint2*)(((unsigned long long)wave_uniform(r0.w) << 32) | wave_uniform(r0.z)),
                                    (const ZrInstance*)(((unsigned long long)wave_uniform(r1.y) << 32) | wave_uniform(r1.x)),
                                    wave_uniform(r1.z), wave_uniform(r1.w) };      // the record's words, made known-uniform
            const MeshletHead H = meshlet_head(P.PVM, be, lane);
            const uint32_t tcount = H.tcount;
            const uint2 tri_w[2] = { H.tri_w[0], H.tri_w[1] };
            const zf4 c = H.c;
            const float FM = 3.402823466e38f, gb = ZR_GUARD * c.w;
            const bool fin = __builtin_fabsf(c.x) <= FM && __builtin_fabsf(c.y) <= FM && __builtin_fabsf(c.z) <= FM && __builtin_fabsf(c.w) <= FM;
            const bool odd = !fin || c.x < -c.w || c.x > c.w || c.y < -c.w || c.y > c.w || c.z < 0.0f || c.z > c.w ||
                             !(c.w > 0.0f) || __builtin_fabsf(c.x) > gb || __builtin_fabsf(c.y) > gb;
            const bool flagged = __ballot(lane < H.vcount && odd) != 0ull;
            if (lane < H.vcount) {
                const uint32_t f = flagged ? vertex_flags(c) : 0u;
                SV s; s.X = 0; s.Y = 0; s.z = 0.0f; s.rw = 0.0f;
                if (!(f & 129u)) s = project(c, P.hw, P.hh);
                vstage[wv][lane] = make_int4(s.X - ox, s.Y - oy, (int)zr_f2u(s.z), (int)f);      // snapped x, y (tile-relative), depth, clip flags
            }
            lds_fence();

            // phase 1: every triangle gets the cheap tests; survivors are compacted into this wave's LDS ring so that
            // phase 2 (setup + pixel walk) always runs with full lanes, across meshlet boundaries
#pragma unroll
            for (int round = 0; round < 2; ++round) {
                const uint32_t t0 = (uint32_t)round * WAVE;
                if (t0 >= tcount || ZR_DIAG_SKIP(P.debug_skip) >= 2u) break;
                const uint32_t t = t0 + lane;
                bool alive = false;
                int4 r0 = make_int4(0, 0, 0, 0), r1 = r0, r2 = r0;
                const uint32_t prim = H.pbase + tri_w[round].y;
                if (t < tcount) {
                    const uint32_t i0 = tri_w[round].x & 255u, i1 = (tri_w[round].x >> 8) & 255u, i2 = (tri_w[round].x >> 16) & 255u;
                    r0 = vstage[wv][i0]; r1 = vstage[wv][i1]; r2 = vstage[wv][i2];
                    int cls = flagged ? classify((uint32_t)r0.w, (uint32_t)r1.w, (uint32_t)r2.w) : 1;
                    // a triangle with an edge of 64 pixels or more goes the clipper's way too: that route holds the 64-bit walk
                    // (it leaves a triangle that needs no clipping as it is, so the pixels are the same) - but only for the windows its
                    // snapped box reaches: a ground triangle under a 2048^2 map is met in thousands of tiles' lists and touches a few
                    if (cls == 1 && !tri_is_small(r0.x, r0.y, r1.x, r1.y, r2.x, r2.y))
                        cls = tri_prefilter(r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, T) ? 2 : 0;
                    if (cls == 1) alive = tri_prefilter(r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, T);
                    else if (cls == 2) {
                        zf4 cc[3];      // (transformed before the place is claimed; k_geom's writer claims first: see DESIGN App. A)
                        const uint32_t li[3] = { i0, i1, i2 };
                        for (int k = 0; k < 3; ++k) {
                            const float4 pk = ld_global(H.mp + li[k]);
                            cc[k] = zr_mat4_point(P.PVM, vs_position(zr3(pk.x, pk.y, pk.z), H.I, H.instanced));
                        }
                        const uint32_t pos = atomicAdd(&stats->n_slow[0], 1u);          // rare: one atomic apiece does
                        if (pos < slow_cap) {
                            for (int k = 0; k < 3; ++k) slow[4u * pos + (uint32_t)k] = make_uint4(zr_f2u(cc[k].x), zr_f2u(cc[k].y), zr_f2u(cc[k].z), zr_f2u(cc[k].w));
                            slow[4u * pos + 3u] = make_uint4(prim, tile, 0u, 0u);
                        } else { stats->overflow = 1u; stats->overflow_sticky = ZR_OVF_SLOW; }
                    }
                }
                const unsigned long long mask = __ballot(alive);
                if (alive) {
                    const uint32_t slot = (qhead + qn + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))) & (QCAP - 1u);
                    int* q = &queue[wv][0][slot];
                    q[0 * QCAP] = (r0.x & 0xFFFF) | (r0.y << 16); q[1 * QCAP] = r0.z;
                    q[2 * QCAP] = (r1.x & 0xFFFF) | (r1.y << 16); q[3 * QCAP] = r1.z;
                    q[4 * QCAP] = (r2.x & 0xFFFF) | (r2.y << 16); q[5 * QCAP] = r2.z;
                    q[6 * QCAP] = (int)prim;
                }
                qn += (uint32_t)__popcll(mask);
                if (ZR_DIAG_SKIP(P.debug_skip) >= 1u) { qhead = (qhead + qn) & (QCAP - 1u); qn = 0; }
                if (qn >= WAVE) {
                    lds_fence();
                    queue_draw(&queue[wv][0][(qhead + lane) & (QCAP - 1u)], T, keys32);
                    qhead = (qhead + WAVE) & (QCAP - 1u); qn -= WAVE;
                }
            }
        }
        if (qn) {      // flush the tail of this chunk
            lds_fence();
            if (lane < qn) queue_draw(&queue[wv][0][(qhead + lane) & (QCAP - 1u)], T, keys32);
            qhead = (qhead + qn) & (QCAP - 1u); qn = 0;
        }
        __syncthreads();
        keys_merge(P, tpx0, tpy0, keys32, shadow_bits, tid, RTHREADS);
        // the next unit, as claim_unit (zr_raster.h) hands them out, but for its last barrier: the keys are re-cleared, behind one, at the
        // top of the loop (spelled out: through the helper the kernel's scalar registers are allocated differently)
        if (first) { first = false; __syncthreads(); chunk += gridDim.x; continue; }
        if (tid == 0) cur_chunk = 2u * gridDim.x + atomicAdd(&stats->chunk_counter[LATE ? 1 : 0], 1u);
        __syncthreads();
        chunk = cur_chunk;
    }
}

// The slow triangles of the pass (they need the clipper, or have an edge of 64 px or more): every tile draws the ones its list named
// through raster_clipped.  A SMALL persistent grid (ZR_SLOW_BLOCKS workgroups stride over the tiles): the usual pass has no slow triangle,
// and as one workgroup per tile the launch cost tens of microseconds just to find room beside the other lane's kernels and return.
#ifndef ZR_SLOW_BLOCKS
#define ZR_SLOW_BLOCKS 256u
#endif
__global__ __launch_bounds__(256) void k_shadow_slow(ZrPass P, const uint32_t* __restrict__ tiles, uint32_t n_tiles, const uint4* __restrict__ slow,
                                                     uint32_t slow_cap, ZrDevStats* __restrict__ stats, uint32_t* __restrict__ shadow_bits)
{
    __shared__ uint32_t keys32[SPAN_PIX(ZR_MODE_SHADOW)];
    const uint32_t n_slow = min(stats->n_slow[0], slow_cap);
    if (n_slow == 0u) return;
    const uint32_t tid = threadIdx.x;
    for (uint32_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const uint32_t tile = tiles[ti];
        keys_clear(keys32, tid, 256u);
        __syncthreads();
        int tpx0, tpy0;
        const TileCtx T = tile_ctx(P, tile, tpx0, tpy0);
        for (uint32_t j = tid; j < n_slow; j += 256u) {
            const uint4 q3 = slow[4u * j + 3u];
            if (q3.y != tile) continue;          // (the rasteriser lists a triangle once per tile of its meshlet)
            zf4 c0, c1, c2;
            slow_read(slow, j, c0, c1, c2);
            raster_clipped<ZR_MODE_SHADOW>(c0, c1, c2, q3.x, T, P.hw, P.hh, tpx0 * 256, tpy0 * 256, nullptr, keys32);
        }
        __syncthreads();
        keys_merge(P, tpx0, tpy0, keys32, shadow_bits, tid, 256u);
        __syncthreads();      // the keys are cleared again for the next tile
    }
}

// Occlusion culling of the shadow pass.  The map is a running minimum: a meshlet-instance whose least possible depth lies behind EVERY texel
// its box can reach, at any moment of the pass, cannot change the map - then or later - and need not be drawn; what is drawn is the same
// whatever was left out, so the map is bit for bit the one the full pass writes.  Which ones to try first is a guess taken from the
// previous frame (one byte per work item): the rasteriser's first launch draws the flagged ones (everything, on a scene's first frame),
// then this kernel tests EVERY survivor of the cull against the map as it stands (box and least depth from k_cull_box: conservative, the
// camera pass's Hi-Z bounds), flags "not hidden" for the next frame, and hands the unflagged ones that are not hidden to a late launch
// of the rasteriser.  A light or a scene that moves costs late work, never a wrong texel.
// A wave takes 64 survivors of the cull, a lane each for the item's record (box, least depth, flag), and writes their flags with ONE store
// (a byte stored per item by whichever lane happened to test it is a partial write of a cache line that lanes of other waves write too:
// 110 000 of those took 150 us).  The texels are read by TASKS: one per (item, row of its box), dealt out to the lanes by a prefix sum
// over the boxes' heights, so a 4 x 4 box costs 4 lane-loads and a 40 x 40 one 400, whatever mix a wave meets.  A task loads its row in
// spans of 4 texels (the map's rows are 4-byte aligned, nothing more is asked of a global load), masks what lies beyond the box's right
// edge, and folds its maximum into the item's word in LDS (ds_max).
struct __attribute__((packed, aligned(4))) ZrTexel4 { uint32_t x, y, z, w; };      // four texels of a map row, from any texel on
template <bool WORKLIST>
__global__ __launch_bounds__(256) void k_shadow_occlusion(ZrPass P, const ZrObject* __restrict__ objs, const uint32_t* __restrict__ work,
                                                          const uint32_t* __restrict__ rects, const uint2* __restrict__ pxrect,
                                                          const float* __restrict__ zmin, uint8_t* __restrict__ flags,
                                                          const uint32_t* __restrict__ shadow_bits, ZrBinEntry* __restrict__ bins,
                                                          ZrDevStats* __restrict__ stats, uint32_t retest)
{
    // retest: which quarter of the FLAGGED items is tested this frame (work id + retest divisible by 4; >= 4: all of them, a scene's first
    // frame).  A flagged item was drawn by the first launch whatever the test says - the test only decides whether it is drawn again next
    // frame - so it can wait up to three frames; an unflagged item is tested every frame (it is drawn if the test does not hide it).
    __shared__ uint32_t s_first[4][WAVE], s_far[4][WAVE];      // per wave: an item's first task, the farthest texel of its box so far
    __shared__ uint2 s_box[4][WAVE];
    // A workgroup takes 1 024 consecutive work items and first lists the survivors of the cull among them (a quarter, at 1 M instances):
    // the waves then work on full sets of 64 survivors.  (A wave's stretch is a chain of three or four dependent round trips to memory, and
    // 8 waves per SIMD is all there is to hide it: with the dead items in the lanes the kernel took 300 us for 11 M items, 2.75 M alive.)
    __shared__ uint32_t s_live[1024], s_nlive;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t n = WORKLIST ? stats->n_vis_work[0] : P.n_work;
    uint32_t n_occl = 0, n_late = 0;
    for (uint32_t blk = blockIdx.x * 1024u; blk < n; blk += gridDim.x * 1024u) {
      if (threadIdx.x == 0u) s_nlive = 0u;
      __syncthreads();
      {
        uint32_t rr[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) { const uint32_t k = blk + j * 256u + threadIdx.x; rr[j] = k < n ? rects[k] : ZR_RECT_CULLED; }
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const unsigned long long m = __ballot(rr[j] != ZR_RECT_CULLED);
            uint32_t at = 0;
            if (lane == 0u && m) at = atomicAdd(&s_nlive, (uint32_t)__popcll(m));
            at = lane_bcast(at, 0u);
            if (rr[j] != ZR_RECT_CULLED) s_live[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = blk + j * 256u + threadIdx.x;
        }
      }
      __syncthreads();
      const uint32_t n_live = s_nlive;
      for (uint32_t base = wv * 64u; base < n_live; base += 256u) {
        const bool have = base + lane < n_live;
        const uint32_t k = have ? s_live[base + lane] : 0u;
        uint32_t r = ZR_RECT_CULLED, w = 0, zb = 0x80000000u;
        uint2 pr = make_uint2(0u, 0u);
        bool flagged = true;
        if (have) {
            r = rects[k]; pr = pxrect[k]; zb = zr_f2u(zmin[k]); w = WORKLIST ? work[k] : k;
            flagged = flags[w] != 0;
        }
        const bool live = r != ZR_RECT_CULLED;
        const uint32_t x0 = pr.x & 0xFFFFu, y0 = pr.x >> 16, x1 = pr.y & 0xFFFFu, y1 = pr.y >> 16;
        // (zmin < 0: the box touches the near plane or the guard band, or is not finite: drawn, never tested; boxes wider than 64 texels neither)
        const bool due = !flagged || retest >= 4u || ((w + retest) & 3u) == 0u;
        const bool test = live && due && (int)zb >= 0 && x1 - x0 < 64u && y1 - y0 < 64u;
        const uint32_t rows = test ? y1 - y0 + 1u : 0u;
        const uint32_t incl = wave_incl_scan(rows), total = lane_bcast(incl, 63u);
        lds_fence();      // the previous stretch's readers are done
        s_first[wv][lane] = incl - rows; s_far[wv][lane] = 0u; s_box[wv][lane] = pr;
        lds_fence();
        for (uint32_t t0 = 0; t0 < total; t0 += 64u) {
            const uint32_t t = t0 + lane;
            if (t < total) {
                // the item this task belongs to: the last one whose first task is <= t (items without rows share their successor's first task)
                uint32_t i = 0;
#pragma unroll
                for (uint32_t step = 32u; step; step >>= 1) if (s_first[wv][i + step] <= t) i += step;
                const uint2 b = s_box[wv][i];
                const uint32_t bx0 = b.x & 0xFFFFu, bx1 = b.y & 0xFFFFu, y = (b.x >> 16) + (t - s_first[wv][i]);
                const uint32_t* __restrict__ row = shadow_bits + (size_t)y * P.W;
                uint32_t far = 0;
                for (uint32_t x = bx0; x <= bx1; x += 4u) {
                    const uint32_t xs = min(x, P.W - 4u);
                    const ZrTexel4 v = *(const ZrTexel4*)(row + xs);
                    if (xs >= bx0 && xs <= bx1) far = max(far, v.x);
                    if (xs + 1u >= bx0 && xs + 1u <= bx1) far = max(far, v.y);
                    if (xs + 2u >= bx0 && xs + 2u <= bx1) far = max(far, v.z);
                    if (xs + 3u >= bx0 && xs + 3u <= bx1) far = max(far, v.w);
                }
                atomicMax(&s_far[wv][i], far);
            }
        }
        lds_fence();
        const bool hidden = test && zb > s_far[wv][lane];        // depth bits of [0, 1]: ordered as integers
        if (live) flags[w] = hidden ? 0u : 1u;
        if (live && !flagged && hidden) ++n_occl;
        if (live && !flagged && !hidden) {
            // late: one self-contained record per (tile, meshlet-instance), as k_bin_fill writes them, with the tile in prim_base
            ++n_late;
            ZrBinEntry be = bin_entry(objs, (int)P.n_objects, w);
            const uint32_t room = P.bin_capacity - min(stats->bin_entries[0], P.bin_capacity);      // above the first launch's entries
            const TileRect R = rect_unpack(r);
            for (uint32_t ty = R.ty0; ty <= R.ty1; ++ty)
                for (uint32_t tx = R.tx0; tx <= R.tx1; ++tx) {
                    const uint32_t pos = atomicAdd(&stats->n_chunks[1], 1u);      // (late entries are few; a light that jumps pays ~10 ns apiece here)
                    be.prim_base = ty * P.tiles_x + tx;
                    if (pos < room) bins[P.bin_capacity - 1u - pos] = be;
                    else { stats->overflow = 1u; stats->overflow_sticky = ZR_OVF_LATE; }
                }
        }
      }
      __syncthreads();      // the list is rewritten by the next stretch
    }
    // the tally in 32 partial sums (the shadow pipeline's block has no other use for covered_part; zr_finish adds them up): one atomic per
    // workgroup on ONE word queued up for ~10 ns apiece - 17 us for config 3's 1 719 workgroups
    n_occl = (uint32_t)wave_sum((int)n_occl); n_late = (uint32_t)wave_sum((int)n_late);
    if (lane == 0u) {
        if (n_occl) atomicAdd(&stats->covered_part[(blockIdx.x * 4u + wv) & 31u], n_occl);
        if (n_late) atomicAdd(&stats->shadow_late, n_late);
    }
}

// statistics only (not part of the frame): shadow-map texels with depth < 1
__global__ void k_count_shadow(const uint32_t* __restrict__ bits, size_t n, ZrDevStats* __restrict__ stats)
{
    uint32_t c = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) c += bits[i] != 0x3F800000u;
    for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&stats->covered_shadow, c);
}

// ------------------------------------------------------------------------------------------------ launchers (C++ linkage, used by zr_frame_host.cpp)

void zr_launch_bin_count(const ZrPass& P, const uint32_t* work, const uint32_t* rects, uint32_t* tile_count, const ZrHiz& Z, const ZrDevStats* stats,
                         hipStream_t s)
{
    if (P.n_work == 0) return;
    const uint32_t n_tiles = P.tiles_x * P.tiles_y;
    hipLaunchKernelGGL(k_bin_count, dim3((P.n_work + 1023) / 1024), dim3(1024), n_tiles * sizeof(uint32_t), s, P, work, rects, tile_count, Z, stats);
}
void zr_launch_scan(uint32_t* tile_count, uint32_t* tile_offset, uint32_t* tile_cursor, uint32_t* chunk_offset, uint4* chunk_tab,
                    uint32_t chunk_cap, uint32_t n, uint32_t capacity, ZrDevStats* stats, hipStream_t s,
                    uint32_t chunk)
{
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, s, tile_count, tile_offset, tile_cursor, chunk_offset, chunk_tab, chunk_cap, n, capacity, stats, chunk);
}
void zr_launch_bin_fill(const ZrPass& P, const ZrObject* objs, const uint32_t* work, const uint32_t* rects, const uint32_t* tile_offset,
                        uint32_t* tile_cursor, ZrBinEntry* bins, const ZrHiz& Z, ZrDevStats* stats, hipStream_t s)
{
    if (P.n_work == 0) return;
    const uint32_t n_tiles = P.tiles_x * P.tiles_y;
    hipLaunchKernelGGL(k_bin_fill, dim3((P.n_work + 1023) / 1024), dim3(1024), n_tiles * sizeof(uint32_t), s, P, objs, work, rects,
                       tile_offset, tile_cursor, bins, Z, stats);
}
void zr_launch_raster_chunks(const ZrPass& P, const ZrObject* objs, const uint4* chunk_tab, const ZrBinEntry* bins, ZrDevStats* stats,
                             uint32_t* shadow_bits, uint32_t n_blocks, hipStream_t s, uint4* slow, uint32_t slow_cap, const uint32_t* tiles,
                             uint32_t n_tiles, int stage)
{
    if (stage == 2) hipLaunchKernelGGL(k_raster_chunks<true>, dim3(n_blocks), dim3(RTHREADS), 0, s, P, objs, chunk_tab, bins, stats, shadow_bits, slow, slow_cap);
    else hipLaunchKernelGGL(k_raster_chunks<false>, dim3(n_blocks), dim3(RTHREADS), 0, s, P, objs, chunk_tab, bins, stats, shadow_bits, slow, slow_cap);
    if (n_tiles && stage != 1) hipLaunchKernelGGL(k_shadow_slow, dim3(std::min<uint32_t>(n_tiles, ZR_SLOW_BLOCKS)), dim3(256), 0, s, P, tiles, n_tiles, slow, slow_cap, stats, shadow_bits);
}
void zr_launch_shadow_occlusion(const ZrPass& P, const ZrObject* objs, const uint32_t* work, const uint32_t* rects, const uint2* pxrect,
                                const float* zmin, uint8_t* flags, const uint32_t* shadow_bits, ZrBinEntry* bins, ZrDevStats* stats,
                                uint32_t n_blocks, uint32_t retest, hipStream_t s)
{
    if (P.n_work == 0) return;
    const dim3 g(std::min<uint32_t>((P.n_work + 1023u) / 1024u, n_blocks)), b(256);
    if (P.use_worklist) hipLaunchKernelGGL(k_shadow_occlusion<true>, g, b, 0, s, P, objs, work, rects, pxrect, zmin, flags, shadow_bits, bins, stats, retest);
    else hipLaunchKernelGGL(k_shadow_occlusion<false>, g, b, 0, s, P, objs, work, rects, pxrect, zmin, flags, shadow_bits, bins, stats, retest);
}
void zr_launch_count_shadow(const uint32_t* bits, size_t n, ZrDevStats* stats, hipStream_t s)
{
    hipLaunchKernelGGL(k_count_shadow, dim3(256), dim3(256), 0, s, bits, n, stats);
}
