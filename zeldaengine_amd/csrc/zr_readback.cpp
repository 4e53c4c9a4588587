// zr_readback.cpp — what a host reads back behind the C-ABI (zelda_render.h): zr_finish, statistics, pass times, latencies and periods,
// the frame's targets, the identity queries (zr_ctx::ids) and the packed tile buffer of a multi-GPU rank.
#include "zr_ctx.h"

#include <algorithm>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <cstdlib>

// The shadow pipeline's block: its slot-0 counters and its overflow latch belong to the frame's statistics
static void merge_shadow_stats(zr_ctx* c, const ZrDevStats& sh)
{
    ZrDevStats& h = c->h_stats;
    h.survivors[0] = sh.survivors[0]; h.bin_entries[0] = sh.bin_entries[0]; h.n_chunks[0] = sh.n_chunks[0];
    h.n_slow[0] = sh.n_slow[0]; h.n_vis_work[0] = sh.n_vis_work[0];
    // (k_shadow_occlusion tallies in 32 partial sums; survivors of the cull = drawn by the first launch + left out + drawn late)
    h.shadow_occluded = 0; for (uint32_t v : sh.covered_part) h.shadow_occluded += v;
    h.shadow_late = sh.shadow_late;
    h.survivors[0] += h.shadow_occluded + h.shadow_late;
    h.overflow |= sh.overflow;
    if (!h.overflow_sticky) h.overflow_sticky = sh.overflow_sticky;      // (a ZR_OVF_* code: the camera lane's, else the pipeline's)
}

extern "C" int zr_finish(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        // (a newest frame that recorded no end of its own gets it here, ahead of the wait: the periods' last run ends where the GPU did)
        hipEvent_t end;
        if (c->frame_no >= 1) { if (int rc = zr_frame_end(c, c->frame_no - 1, &end)) return rc; }
        HIPCHK(c, zr_sync_all(c));
        if (c->rendered) {
            HIPCHK(c, hipMemcpy(&c->h_stats, c->d_stats, sizeof(ZrDevStats), hipMemcpyDeviceToHost));
            if (c->cov_block != c->d_stats)       // the newest frame's resolve ran on the host's stream and counted into its own block
                HIPCHK(c, hipMemcpy(c->h_stats.covered_part, c->cov_block->covered_part, sizeof c->h_stats.covered_part, hipMemcpyDeviceToHost));
            ZrDevStats sh;
            HIPCHK(c, hipMemcpy(&sh, c->d_sstats, sizeof(ZrDevStats), hipMemcpyDeviceToHost));
            merge_shadow_stats(c, sh);
            c->h_stats.covered_shadow = 0;
            if (c->h_stats.overflow_sticky) {     // latched by ANY frame since the last zr_finish, not only the newest one
                HIPCHK(c, zr_fill_sync({ { &c->d_stats->overflow_sticky, 0, sizeof(uint32_t) }, { &c->d_sstats->overflow_sticky, 0, sizeof(uint32_t) } }));
                c->h_stats.overflow = 1u;
                // (a frame that ran full may have left an incomplete key buffer, and a rest would stand on it: the next frame draws round 2
                // again, from buckets planned from this frame's counts, and heals as it did before round 2 was ever kept)
                zr_camera_changed(c);
                static const char* const what[] = { "?", "shadow bin entries", "slow-triangle list (zr_set_limits)", "camera work-unit table", "triangle-record arrays (zr_set_limits)",
                                                    "late shadow bin entries" };
                const uint32_t code = c->h_stats.overflow_sticky < 6u ? c->h_stats.overflow_sticky : 0u;
                char msg[160];
                snprintf(msg, sizeof msg, "tile bin list overflow (%s): a frame since the last zr_finish is incomplete", what[code]);
                return zr_fail(c, ZR_ERR_OVERFLOW, msg);
            }
        }
        return ZR_OK;
    });
}

static_assert(ZRT_CULL_SHADOW == (int)ZR_PASS_CULL_SHADOW && ZRT_SHADOW == (int)ZR_PASS_SHADOW && ZRT_CULL_CAMERA == (int)ZR_PASS_CULL_CAMERA &&
              ZRT_GBUFFER == (int)ZR_PASS_GBUFFER && ZRT_HIZ == (int)ZR_PASS_HIZ && ZRT_GBUFFER2 == (int)ZR_PASS_GBUFFER2 && ZRT_RESOLVE == (int)ZR_PASS_RESOLVE &&
              ZRT_LIGHTING == (int)ZR_PASS_LIGHTING && ZRT_COMPOSITE == (int)ZR_PASS_COMPOSITE && ZRT_TOTAL == (int)ZR_PASS_TOTAL && ZRT_COUNT == (int)ZR_PASS_COUNT,
              "zr_timed.h: the figures are zelda_render.h's ZR_PASS_*");
// One figure of one sample, by the rule stored with it (zr_timed.h): the sum of its spans, each between two events this sample recorded, or
// exactly 0 for a stage the frame did not run - an event of another sample, still in the ring's slot, is never asked about.
static int timed_figure(zr_ctx* c, const zr_ctx::TimedFrame& T, int figure, float* ms)
{
    const ZrTimedReading& g = T.rule.fig[figure];
    *ms = 0.0f;
    for (int i = 0; i < g.n; ++i) {
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, T.ev[g.span[i].from], T.ev[g.span[i].to]));
        *ms += t;
    }
    return ZR_OK;
}

// Mean per-pass GPU time over the last `last_n` frames (<= EV_RING), from hipEvents recorded on the render stream.
extern "C" int zr_get_pass_times_avg(zr_ctx* c, uint32_t last_n, float ms[ZR_PASS_COUNT])
{
    if (!c || !ms) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!c->rendered) return zr_fail(c, ZR_ERR_STATE, "nothing rendered yet");
        int rc = zr_finish(c);
        if (rc && rc != ZR_ERR_OVERFLOW) return rc;
        if (last_n == 0) last_n = 1;
        if (last_n > (uint32_t)zr_ctx::EV_RING) last_n = zr_ctx::EV_RING;
        if (c->sample_no == 0) return zr_fail(c, ZR_ERR_STATE, "no timed frame yet (zr_set_timing_interval)");
        if ((uint64_t)last_n > c->sample_no) last_n = (uint32_t)c->sample_no;
        double acc[ZR_PASS_COUNT] = { 0 };
        for (uint32_t k = 0; k < last_n; ++k) {
            const zr_ctx::TimedFrame& T = c->timed[(c->sample_no - 1 - k) % zr_ctx::EV_RING];
            for (int i = 0; i < ZR_PASS_COUNT; ++i) {
                float t = 0.0f;
                if (int rc2 = timed_figure(c, T, i, &t)) return rc2;
                acc[i] += t;
            }
        }
        for (int i = 0; i < ZR_PASS_COUNT; ++i) ms[i] = (float)(acc[i] / last_n);
        return ZR_OK;
    });
}
extern "C" int zr_get_pass_times(zr_ctx* c, float ms[ZR_PASS_COUNT]) { return zr_guard(c, [&]() -> int { return zr_get_pass_times_avg(c, 1, ms); }); }

// Begin-to-end GPU time (first kernel of the camera lane to the end of the lighting pass) of each of the last `n` timed frames,
// newest first; returns how many were written.  With two frames in flight this latency is longer than the frame period.
extern "C" int zr_get_frame_latencies(zr_ctx* c, uint32_t n, float* ms)
{
    if (!c || !ms) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!c->rendered) return zr_fail(c, ZR_ERR_STATE, "nothing rendered yet");
        int rc = zr_finish(c);
        if (rc && rc != ZR_ERR_OVERFLOW) return rc;
        if (n > (uint32_t)zr_ctx::EV_RING) n = zr_ctx::EV_RING;
        if ((uint64_t)n > c->sample_no) n = (uint32_t)c->sample_no;
        for (uint32_t k = 0; k < n; ++k)
            if (int rc2 = timed_figure(c, c->timed[(c->sample_no - 1 - k) % zr_ctx::EV_RING], ZR_PASS_TOTAL, &ms[k])) return rc2;
        return (int)n;
    });
}

// GPU time between the ends of consecutive frames (the frame period the GPU sustained) for the last `n` frames, newest first;
// returns how many were written (<= END_RING - 1).  Costs nothing extra: the end-of-frame event exists for the double buffering.
// Frames inside a run of one-launch frames record no end of their own (zr_frame_end.h): every frame between two recorded ends reports
// the mean of its run, and the sum over a window whose ends are recorded is exact.
extern "C" int zr_get_frame_periods(zr_ctx* c, uint32_t n, float* ms)
{
    if (!c || !ms) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!c->rendered) return zr_fail(c, ZR_ERR_STATE, "nothing rendered yet");
        int rc = zr_finish(c);
        if (rc && rc != ZR_ERR_OVERFLOW) return rc;
        const uint64_t have = c->frame_no > 0 ? c->frame_no - 1 : 0;
        if (n > (uint32_t)zr_ctx::END_RING - 1u) n = zr_ctx::END_RING - 1;
        if ((uint64_t)n > have) n = (uint32_t)have;
        for (uint32_t k = 0; k < n; ++k) {
            uint64_t a = 0, b = 0;
            if (!zr_end_run(c->end, c->frame_no - 1 - k, &a, &b)) return (int)k;      // (its run reaches out of the ring: the frames so far)
            float run = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&run, c->ev_end[a % zr_ctx::END_RING], c->ev_end[b % zr_ctx::END_RING]));
            ms[k] = run / (float)(b - a);
        }
        return (int)n;
    });
}

// Per-pass hipEvents are recorded on every interval-th frame (default 1 = every frame, 0 = never).  Each record is a small
// bubble on the stream it sits on (~6 us on MI355X; a frame records the events of the stages it runs: zr_timed.h), so a host that only
// wants throughput samples sparsely.
extern "C" int zr_set_timing_interval(zr_ctx* c, uint32_t interval)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        c->timing_interval = interval;
        return ZR_OK;
    });
}


// `bytes` = sizeof(zr_stats) as the CALLER was compiled: the struct only ever grows at its end, so a host built against an older header
// gets the fields it knows and is never written past.
extern "C" int zr_get_stats(zr_ctx* c, zr_stats* out_user, size_t bytes)
{
    if (!c || !out_user) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, bytes >= offsetof(zr_stats, round1_survivors) && bytes % 4 == 0);      // (the first release's struct ended there)
        zr_stats out_full; zr_stats* out = &out_full;
        int rc = zr_finish(c);
        if (c->rendered && (rc == ZR_OK || rc == ZR_ERR_OVERFLOW)) {      // shadow coverage is a statistic, counted on demand
            ZrDevStats z; (void)hipMemcpy(&z, c->d_stats, sizeof z, hipMemcpyDeviceToHost);
            uint32_t zero = 0;
            (void)hipMemcpy(&c->d_stats->covered_shadow, &zero, 4, hipMemcpyHostToDevice);
            zr_launch_count_shadow((const uint32_t*)shadow_buf(c), (size_t)c->SD * c->SD, c->d_stats, c->stream);
            (void)hipStreamSynchronize(c->stream);
            // (the count is the one word of the block that changed since zr_finish read it and merged the shadow pipeline's into it)
            (void)hipMemcpy(&c->h_stats.covered_shadow, &c->d_stats->covered_shadow, 4, hipMemcpyDeviceToHost);
        }
#ifdef ZR_DIAG
        if (getenv("ZR_DUMP_STATS")) {     // diagnostics: the raw device block
            const ZrDevStats& h = c->h_stats;
            fprintf(stderr, "zr stats: survivors %u %u %u  bin_entries %u %u %u  n_sel %u %u %u  n_slow %u %u %u  hiz_culled %u  n_chunks %u %u %u  overflow records %u %u\n",
                    h.survivors[0], h.survivors[1], h.survivors[2], h.bin_entries[0], h.bin_entries[1], h.bin_entries[2], h.n_sel[0], h.n_sel[1], h.n_sel[2],
                    h.n_slow[0], h.n_slow[1], h.n_slow[2], h.hiz_culled, h.n_chunks[0], h.n_chunks[1], h.n_chunks[2], h.pool_used[1], h.pool_used[2]);
        }
#endif
        memset(out, 0, sizeof *out);
        for (int i = 0; i < 2; ++i) {
            out->work_items[i] = c->last_work[i]; out->survivors[i] = c->h_stats.survivors[i]; out->bin_entries[i] = c->h_stats.bin_entries[i];
        }
        out->survivors[1] += c->h_stats.survivors[2]; out->bin_entries[1] += c->h_stats.bin_entries[2];    // both rounds of the camera pass
        out->hiz_culled = c->h_stats.hiz_culled; out->round1_survivors = c->last_two_round ? c->h_stats.survivors[1] : 0;
        out->covered_pixels = 0; for (uint32_t v : c->h_stats.covered_part) out->covered_pixels += v;
        out->covered_shadow_texels = c->h_stats.covered_shadow; out->overflow = c->h_stats.overflow;
        out->shadow_occluded = c->h_stats.shadow_occluded; out->shadow_late = c->h_stats.shadow_late;
        out->hiz_culled_geom = c->h_stats.hiz_culled_geom; out->struct_bytes = (uint32_t)sizeof(zr_stats);
        memcpy(out_user, out, std::min(bytes, sizeof(zr_stats)));
        return rc;
    });
}

// ------------------------------------------------------------------------------------------------ read-back

extern "C" int zr_read_color(zr_ctx* c, uint8_t* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, dst && bytes == (size_t)c->W * c->H * 4);
        int rc = zr_finish(c);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(dst, c->d_color, bytes, hipMemcpyDeviceToHost));
        return ZR_OK;
    });
}
extern "C" int zr_read_gbuffer(zr_ctx* c, int target, void* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        const GBufferPtrs& G = c->fc[c->fcur].G;
        const void* src[6] = { G.depth, G.scene_color, G.gA, G.gB, G.gC, G.gD };
        ARGCHK(c, dst && target >= 0 && target < 6);
        ARGCHK(c, bytes == (size_t)c->W * c->H * (target == 5 ? 8 : 4));
        int rc = zr_finish(c);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(dst, src[target], bytes, hipMemcpyDeviceToHost));
        return ZR_OK;
    });
}
extern "C" int zr_read_shadowmap(zr_ctx* c, float* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, dst && bytes == (size_t)c->SD * c->SD * 4);
        int rc = zr_finish(c);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(dst, shadow_buf(c), bytes, hipMemcpyDeviceToHost));
        return ZR_OK;
    });
}

// The frame enqueued last, copied into caller-owned DEVICE buffers in stream order (no host synchronisation): what a host with two frames
// in flight uses instead of zr_read_color - the copies are ordered behind that frame's lighting pass and ahead of whatever the next
// zr_render enqueues on the render stream.  Either pointer may be NULL.  (The shadow map is double-buffered inside: the NEXT frame's
// shadow pipeline draws into the other copy, so the map copied here is this frame's whatever runs beside it.)
extern "C" int zr_copy_frame_async(zr_ctx* c, void* color_dev, void* shadow_dev)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!c->rendered || c->stage != 0) return zr_fail(c, ZR_ERR_STATE, "zr_copy_frame_async: no finished frame enqueued");
        HIPCHK(c, hipSetDevice(c->device));
        if (color_dev) HIPCHK(c, hipMemcpyAsync(color_dev, c->d_color, (size_t)c->W * c->H * 4, hipMemcpyDeviceToDevice, c->stream));
        if (shadow_dev) HIPCHK(c, hipMemcpyAsync(shadow_dev, shadow_buf(c), (size_t)c->SD * c->SD * 4, hipMemcpyDeviceToDevice, c->stream));
        return ZR_OK;
    });
}

// ------------------------------------------------------------------------------------------------ object identity (zelda_render.h)

// Object identity (zr_set_id_capture): the census's draw table - draw order, as zr_scene_finalize numbers primitives, with each draw's add-order
// object index and first instance slot - and the per-slot arrays of the queries.  Built at the start of a captured frame, when the
// scene's objects changed since.
int ids_prepare(zr_ctx* c)
{
    if (c->ids.table_gen == c->scene_gen && c->ids.draws) return ZR_OK;
    std::vector<uint32_t> slot_base(c->objects.size());
    uint32_t slots = 0;
    for (size_t i = 0; i < c->objects.size(); ++i) { slot_base[i] = slots; slots += c->objects[i].n_inst; }
    std::vector<ZrIdsDraw> tab;
    uint32_t prim = 0;
    for (int pass = 0; pass < 2; ++pass)                 // the draw order of zr_scene_finalize (ZE:3445-3476)
        for (size_t i = 0; i < c->objects.size(); ++i) {
            const ZrSceneObject& o = c->objects[i];
            if ((int)o.instanced != pass) continue;
            const uint32_t nt = (uint32_t)(c->meshes[o.mesh].idx.size() / 3);
            tab.push_back({ prim, nt ? nt : 1u, (uint32_t)i, slot_base[i] });
            prim += nt * o.n_inst;
        }
    tab.push_back({ prim, 1u, 0xFFFFFFFFu, slots });     // sentinel: the end of the last draw
    HIPCHK(c, zr_sync_all(c));                           // (queries of an earlier scene may still read the old table)
    c->ids.table.release(); c->ids.draws = nullptr;
    HIPCHK(c, upload(c->ids.table, &c->ids.draws, tab));
    c->ids.n_draws = (uint32_t)tab.size() - 1u;
    c->ids.n_slots = slots;
    if (slots > c->ids.slot_cap || !c->ids.counts) {
        ZrOwn& P = c->ids.pool;
        P.release(); c->ids.counts = c->ids.cov = c->ids.list = c->ids.n = nullptr; c->ids.keys = nullptr; c->ids.hits = nullptr;
        c->ids.slot_cap = 0;
        const size_t cap = std::max<uint32_t>(slots, 1u);
        HIPCHK(c, P.alloc(&c->ids.counts, cap)); HIPCHK(c, P.alloc(&c->ids.cov, cap)); HIPCHK(c, P.alloc(&c->ids.list, cap));
        HIPCHK(c, P.alloc(&c->ids.n, 1)); HIPCHK(c, P.alloc(&c->ids.keys, cap)); HIPCHK(c, P.alloc(&c->ids.hits, cap));
        // between queries: counts 0, keys all ones, no listed slot (k_id_hits restores this after every pick)
        HIPCHK(c, zr_fill_sync({ { c->ids.counts, 0, cap * 4 }, { c->ids.keys, 0xFF, cap * 8 }, { c->ids.n, 0, 4 } }));
        c->ids.slot_cap = (uint32_t)cap;
    }
    c->ids.table_gen = c->scene_gen;
    return ZR_OK;
}

extern "C" int zr_set_id_capture(zr_ctx* c, int enable)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (int rc = zr_stage_idle(c, "zr_set_id_capture", false)) return rc;
        const bool on = enable != 0;
        if (on == c->id_capture) return ZR_OK;
        HIPCHK(c, hipSetDevice(c->device));
        const int rc = set_winner_planes(c, c->shading == ZR_SHADING_FORWARD, on, "zr_set_id_capture");      // (no drain: frames in flight keep what they were enqueued with)
        if (rc) return rc;
        c->id_capture = on;
        return ZR_OK;
    });
}

// The frame enqueued last kept its winners (capture; a ray cast needs none) and still describes the scene; `sync`: finish it first (its
// overflow is the query's error).
int ids_ready(zr_ctx* c, const char* what, bool sync, bool capture)
{
    if (!c->rendered || c->stage != 0) return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": no finished frame enqueued");
    if (capture && !c->ids_frame) return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": the last frame was rendered without id capture (zr_set_id_capture)");
    if (c->ids.gen != c->scene_gen) return zr_fail(c, ZR_ERR_STATE, std::string(what) + ": the scene changed after the last frame");
    HIPCHK(c, hipSetDevice(c->device));
    return sync ? zr_finish(c) : ZR_OK;
}
int ids_reader_enqueued(zr_ctx* c, bool both)
{
    for (int k = 0; k < 2; ++k) {
        if (!both && k != c->fcur) continue;
        HIPCHK(c, hipEventRecord(c->fc[k].ev_ids, c->stream));
        c->fc[k].ids_wait = true;
    }
    return ZR_OK;
}
ZrIdsArgs ids_args(zr_ctx* c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h)
{
    const FrameCopy& F = c->fc[c->fcur];                      // (stage 0: the copy the frame enqueued last wrote)
    ZrIdsArgs A; memset(&A, 0, sizeof A);
    A.prim = F.prim_plane; A.depth = F.G.depth;
    A.draws = c->ids.draws; A.n_draws = c->ids.n_draws;
    A.W = c->W; A.x0 = x0; A.y0 = y0; A.w = w; A.h = h;
    A.counts = c->ids.counts; A.keys = c->ids.keys; A.hit_list = c->ids.list; A.n_hits = c->ids.n;
    return A;
}

extern "C" int zr_read_ids(zr_ctx* c, int kind, void* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, dst && (kind == ZR_IDS_PRIMITIVE || kind == ZR_IDS_OBJECT));
        ARGCHK(c, bytes == (size_t)c->W * c->H * (kind == ZR_IDS_OBJECT ? 8 : 4));
        int rc = ids_ready(c, "zr_read_ids", true);
        if (rc) return rc;
        const ZrIdsArgs A0 = ids_args(c, 0, 0, c->W, c->H);
        if (kind == ZR_IDS_PRIMITIVE) { HIPCHK(c, hipMemcpy(dst, A0.prim, bytes, hipMemcpyDeviceToHost)); return ZR_OK; }
        if (!c->ids.obj) HIPCHK(c, c->ext.alloc(&c->ids.obj, (size_t)c->W * c->H));
        ZrIdsArgs A = A0; A.obj_plane = c->ids.obj;
        zr_launch_id_census(A, ZR_IDS_OBJECTS, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(dst, c->ids.obj, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return ZR_OK;
    });
}

extern "C" int zr_pick(zr_ctx* c, uint32_t x, uint32_t y, uint32_t w, uint32_t h, zr_hit* hits, uint32_t cap, uint32_t* n)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, n && w > 0 && h > 0 && (hits || cap == 0));
        *n = 0;
        int rc = ids_ready(c, "zr_pick", true);
        if (rc) return rc;
        if (x >= c->W || y >= c->H) return ZR_OK;                  // wholly outside the frame
        ZrIdsArgs A = ids_args(c, x, y, std::min(w, c->W - x), std::min(h, c->H - y));
        zr_launch_id_census(A, ZR_IDS_PICK, c->stream);
        HIPCHK(c, hipGetLastError());
        uint32_t total = 0;
        HIPCHK(c, hipMemcpyAsync(&total, c->ids.n, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (total > c->ids.n_slots) return zr_fail(c, ZR_ERR_DEVICE, "zr_pick: hit list longer than the slot count");
        std::vector<zr_hit> all(total);
        zr_launch_id_hits(A, total, c->ids.hits, c->stream);       // (also clears the listed slots)
        HIPCHK(c, hipGetLastError());
        if (total) HIPCHK(c, hipMemcpyAsync(all.data(), c->ids.hits, sizeof(zr_hit) * total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemsetAsync(c->ids.n, 0, 4, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::sort(all.begin(), all.end(), [](const zr_hit& a, const zr_hit& b) {
            if (a.depth != b.depth) return a.depth < b.depth;
            if (a.object != b.object) return a.object < b.object;
            return a.instance < b.instance;
        });
        if (total) memcpy(hits, all.data(), sizeof(zr_hit) * std::min(total, cap));
        *n = total;
        return ZR_OK;
    });
}

size_t ids_slot_count(const zr_ctx* c)
{
    size_t slots = 0;
    for (const auto& o : c->objects) slots += o.n_inst;      // (n_inst = max(1, instances))
    return slots;
}
static size_t ids_slot_bytes(const zr_ctx* c) { return 4 * ids_slot_count(c); }
// The whole-frame census into a count array on the device (cleared first), on the host's stream.
static int ids_coverage(zr_ctx* c, uint32_t* counts_dev, size_t bytes)
{
    if (bytes) HIPCHK(c, hipMemsetAsync(counts_dev, 0, bytes, c->stream));
    ZrIdsArgs A = ids_args(c, 0, 0, c->W, c->H);
    A.counts = counts_dev;
    if (bytes) zr_launch_id_census(A, ZR_IDS_COVERAGE, c->stream);
    HIPCHK(c, hipGetLastError());
    return ZR_OK;
}
extern "C" int zr_instance_coverage(zr_ctx* c, uint32_t* counts, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, (counts || bytes == 0) && bytes == ids_slot_bytes(c));
        int rc = ids_ready(c, "zr_instance_coverage", true);
        if (rc == ZR_OK) rc = ids_coverage(c, c->ids.cov, bytes);
        if (rc) return rc;
        if (bytes) HIPCHK(c, hipMemcpyAsync(counts, c->ids.cov, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return ZR_OK;
    });
}
extern "C" int zr_instance_coverage_async(zr_ctx* c, void* counts_dev, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, (counts_dev || bytes == 0) && bytes == ids_slot_bytes(c));
        int rc = ids_ready(c, "zr_instance_coverage_async", false);
        if (rc == ZR_OK) rc = ids_coverage(c, (uint32_t*)counts_dev, bytes);
        if (rc) return rc;
        return ids_reader_enqueued(c);      // (the census reads the last frame's winner plane)
    });
}

// ------------------------------------------------------------------------------------------------ multi-GPU tiles

extern "C" int zr_tiles_device_buffer(zr_ctx* c, void** p, size_t* bytes)
{
    if (!c || !p || !bytes) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        *p = c->d_tiles; *bytes = (size_t)c->slots_per_rank * ZR_TILE * ZR_TILE * 4;
        return ZR_OK;
    });
}
// Lets the caller own the packed tile buffer (e.g. a torch tensor handed to RCCL; two of them alternate so that frame k's
// all-gather overlaps frame k+1's rendering).  ptr must hold zr_tiles_device_buffer's byte count; NULL = internal buffer.
extern "C" int zr_set_tiles_buffer(zr_ctx* c, void* ptr)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        c->d_tiles_ext = (uint32_t*)ptr; zr_settle_forget(&c->lk.settle);
        return ZR_OK;
    });
}

extern "C" int zr_read_tiles(zr_ctx* c, uint8_t* dst, size_t bytes)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, dst && bytes == (size_t)c->slots_per_rank * ZR_TILE * ZR_TILE * 4);
        int rc = zr_finish(c);
        if (rc) return rc;
        HIPCHK(c, hipMemcpy(dst, c->d_tiles_ext ? c->d_tiles_ext : c->d_tiles, bytes, hipMemcpyDeviceToHost));
        return ZR_OK;
    });
}
extern "C" int zr_composite(zr_ctx* c, const void* gathered)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, gathered != nullptr);
        HIPCHK(c, hipSetDevice(c->device));
        zr_launch_untile((const uint32_t*)gathered, c->d_tile_map, c->d_color, c->W, c->H, c->tiles_x, c->n_tiles, c->stream);
        zr_settle_forget(&c->lk.settle);      // (it writes the frame: where that is a resting launch's target, nothing stands any more)
        HIPCHK(c, hipGetLastError());
        return ZR_OK;
    });
}
// (the caller may write through it: from here on the context's resting frames write every pixel - zr_ctx::LightKeep::handed_out)
extern "C" int zr_color_device_ptr(zr_ctx* c, void** p)
{
    if (!c || !p) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int { *p = c->d_color; c->lk.handed_out = true; zr_settle_forget(&c->lk.settle); return ZR_OK; });
}
