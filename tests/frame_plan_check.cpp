// frame_plan_check.cpp — the frame schedule (csrc/zr_frame_plan.h) run without a GPU: tests/test_frame_plan.py compiles this file, runs it
// and holds what it prints against expectations written out there.
//
//   1. Scripted sequences of frames through zr_frame_plan / zr_frame_carry, as frame_begin, shadow_pass and gbuffer_pass of
//      zr_frame_host.cpp drive them: "== <name>", then one line of key=value words per frame.
//   2. The invariants of the schedule over every combination of the facts and of the carry's bits, in three sweeps (the shadow map's
//      keep, the camera pass's keeps, the lanes): each sweep takes every combination of the dimensions it names while the others stay at
//      the resting zr_render frame's values.  (One sweep over all 36 dimensions would be 10^13 plans; these three are 2.6 million.)  "swept <name> <combinations>";
//      exit status 1 and a line per broken invariant if one fails.
#include "zr_frame_plan.h"

#include <cstdio>

// ---------------------------------------------------------------------------------------------- a host, without the GPU

// What zr_ctx holds beside the carry, reduced to what the facts are made from: the pass blocks as numbers (equal numbers: equal blocks).
struct Host {
    ZrFrameFacts f;                 // the standing properties, entry and lane; the rest is filled per frame
    ZrFrameCarry k;
    int shadow_block = 1, camera_block = 1;                   // this frame's (the light / the camera moved: another number)
    int smap_key = 0, cam_prev_key = 0, list_key[2] = { 0, 0 };
    uint64_t frame_no = 0, copy_gen[2] = { 0, 0 };
    bool copy_overlay[2] = { false, false };
};

static const char* lane_name(ZrLane l) { return l == ZR_LANE_NONE ? "none" : l == ZR_LANE_HOST ? "host" : "cam"; }
static const char* ev_cam_name(ZrEvCam e)
{
    switch (e) {
    case ZR_EVCAM_NONE: return "none";
    case ZR_EVCAM_BEHIND_MARK: return "mark";
    case ZR_EVCAM_BEHIND_RESOLVE: return "resolve";
    case ZR_EVCAM_BEHIND_ONE_PIXEL: return "one_pixel";
    default: return "lane_end";
    }
}

// One frame, every stage enqueued (zr_render, or the three staged calls in a row).
static void frame(Host& h)
{
    ZrFrameFacts& f = h.f;
    f.frame_no = h.frame_no;
    f.shadow_is_map = h.smap_key == h.shadow_block; f.camera_is_prev = h.cam_prev_key == h.camera_block;
    f.block_is_list[0] = h.list_key[0] == h.shadow_block; f.block_is_list[1] = h.list_key[1] == h.camera_block;
    for (int i = 0; i < 2; ++i) { f.copy_gen[i] = h.copy_gen[i]; f.copy_overlay[i] = h.copy_overlay[i]; }
    const ZrFramePlan p = zr_frame_plan(f, h.k);
    h.k = zr_frame_carry(h.k, f, p, ZR_STAGE_HEAD);
    if (p.shadow_list_rebuild) h.list_key[0] = h.shadow_block;
    if (p.camera_list_rebuild) h.list_key[1] = h.camera_block;
    if (p.shadow != ZR_LANE_NONE) { h.smap_key = h.shadow_block; h.k = zr_frame_carry(h.k, f, p, ZR_STAGE_SHADOW); }
    if (p.camera != ZR_LANE_NONE) {
        const int cur = (int)(h.frame_no & 1u);
        h.copy_overlay[cur] = f.sky; h.copy_gen[cur] = p.g_gen;      // (the resolve, on either stream)
        h.cam_prev_key = h.camera_block; h.k = zr_frame_carry(h.k, f, p, ZR_STAGE_CAMERA);
    }
    printf("frame=%llu head=%s shadow=%s map=%s occlusion=%d shadow_list=%s camera=%s pass=%s count_first=%d hiz=%d camera_list=%s plan_rounds=%d "
           "resolve=%s deferred=%d one_pixel=%s lighting=%s reset_stats=%d reset_list=%d wait_end2=%d wait_end1=%d wait_lane_end=%d wait_ids=%d "
           "ev_cam=%s host_waits=%d ev_join=%d\n",
           (unsigned long long)h.frame_no, lane_name(p.head), lane_name(p.shadow), p.shadow_keep ? "kept" : "drawn", (int)p.shadow_occlusion,
           p.shadow_list_rebuild ? "rebuilt" : p.shadow_list_reuse ? "reused" : "none", lane_name(p.camera),
           p.camera_keep ? "whole" : p.rounds == ZR_ROUNDS_TWO_KEPT ? "round2_kept" : p.rounds == ZR_ROUNDS_TWO ? "two_rounds" : "one_round",
           (int)p.count_first, (int)p.hiz_on, p.camera_list_rebuild ? "rebuilt" : p.camera_list_reuse ? "reused" : "none", (int)p.rounds,
           lane_name(p.resolve), (int)p.resolve_deferred, lane_name(p.one_pixel), lane_name(p.lighting), (int)p.reset_stats, (int)p.reset_camera_list,
           (int)p.wait_end2, (int)p.wait_end1, (int)p.wait_lane_end, (int)p.wait_ids, ev_cam_name(p.ev_cam), (int)p.host_waits_ev_cam, (int)p.ev_join);
    h.frame_no++;
}

// What zr_scene_finalize does to the schedule's state after an edit: history, plan and lists forgotten, casters changed.
static void scene_edit(Host& h)
{
    h.k.vis_history = h.k.plan_valid = h.k.sflag_history = h.k.list_valid[0] = h.k.list_valid[1] = false;
    h.f.caster_epoch++; h.f.camera_epoch++;
}

static Host host(ZrEntry entry, bool has_lane, uint32_t flags = 0)
{
    Host h;
    h.f.flags = flags; h.f.SD = 256; h.f.n_work[0] = h.f.n_work[1] = 1000; h.f.entry = entry; h.f.has_lane = has_lane;
    return h;
}

static void sequences()
{
    const int k = 4;
    { puts("== rest_render"); Host h = host(ZR_ENTRY_RENDER, true); for (int i = 0; i < 8; ++i) frame(h); }
    { puts("== rest_serial"); Host h = host(ZR_ENTRY_RENDER, true, ZRP_SERIAL_PASSES); for (int i = 0; i < 8; ++i) frame(h); }
    { puts("== rest_staged"); Host h = host(ZR_ENTRY_STAGED, true); for (int i = 0; i < 8; ++i) frame(h); }
    { puts("== camera_cut"); Host h = host(ZR_ENTRY_RENDER, true); for (int i = 0; i < 8; ++i) { if (i == k) h.camera_block = 2; frame(h); } }
    { puts("== texture_update"); Host h = host(ZR_ENTRY_RENDER, true); for (int i = 0; i < 8; ++i) { if (i == k) h.f.surface_epoch++; frame(h); } }
    { puts("== light_moves"); Host h = host(ZR_ENTRY_RENDER, true); for (int i = 0; i < 8; ++i) { h.shadow_block = 10 + i; frame(h); } }
    { puts("== light_stops"); Host h = host(ZR_ENTRY_RENDER, true); for (int i = 0; i < 8; ++i) { if (i <= k) h.shadow_block = 10 + i; frame(h); } }
    { puts("== scene_edit"); Host h = host(ZR_ENTRY_RENDER, true); for (int i = 0; i < 8; ++i) { if (i == k) scene_edit(h); frame(h); } }
    { puts("== no_list_reuse"); Host h = host(ZR_ENTRY_RENDER, true, ZRP_NO_LIST_REUSE); h.f.use_worklist[0] = h.f.use_worklist[1] = true; for (int i = 0; i < 8; ++i) frame(h); }
    { puts("== no_hiz"); Host h = host(ZR_ENTRY_RENDER, true, ZRP_NO_HIZ); for (int i = 0; i < 8; ++i) frame(h); }
    { puts("== tile_world_2"); Host h = host(ZR_ENTRY_RENDER, true); h.f.tile_world = 2; h.f.use_worklist[0] = h.f.use_worklist[1] = true; for (int i = 0; i < 8; ++i) frame(h); }
    { puts("== skydome"); Host h = host(ZR_ENTRY_RENDER, true); h.f.sky = true; for (int i = 0; i < 8; ++i) frame(h); }
    {   // two zr_render frames, a staged frame that draws (the camera moved), a zr_render frame again
        puts("== lane_handover"); Host h = host(ZR_ENTRY_RENDER, true);
        frame(h); frame(h);
        h.f.entry = ZR_ENTRY_STAGED; h.camera_block = 2; frame(h);
        h.f.entry = ZR_ENTRY_RENDER; frame(h);
    }
}

// ---------------------------------------------------------------------------------------------- the invariants, over every combination

struct Case { ZrFrameFacts f; ZrFrameCarry k; };

// The resting zr_render frame (frame 3 of rest_render): everything stands, everything is kept.
static Case resting()
{
    Case c;
    c.f.SD = 256; c.f.n_work[0] = c.f.n_work[1] = 1000; c.f.entry = ZR_ENTRY_RENDER; c.f.has_lane = true; c.f.frame_no = 3;
    c.f.caster_epoch = c.f.camera_epoch = c.f.surface_epoch = 7;
    c.f.shadow_is_map = c.f.camera_is_prev = c.f.block_is_list[0] = c.f.block_is_list[1] = true;
    c.f.copy_gen[0] = c.f.copy_gen[1] = 5;
    c.k.smap_valid = c.k.cam_prev_valid = c.k.r2_settled = c.k.plan_valid = c.k.plan_two_round = c.k.vis_history = c.k.sflag_history = true;
    c.k.list_valid[0] = c.k.list_valid[1] = true;
    c.k.smap_epoch = c.k.cam_prev_epoch = c.k.surf_prev_epoch = 7; c.k.smap_frame = 0; c.k.g_gen = 5; c.k.gbuf_lane = ZR_LANE_CAM;
    return c;
}

enum Dim {
    D_NO_HIZ, D_SERIAL, D_NO_LIST_REUSE, D_SHADOW_OCCLUSION, D_NO_SHADOW_OCCLUSION, D_PARTITION, D_MAP_EXTERNAL, D_SKY, D_FORWARD, D_ENTRY,
    D_HAS_LANE, D_FRAME_NO, D_SHADOW_IS_MAP, D_CAMERA_IS_PREV, D_CASTER_EPOCH, D_CAMERA_EPOCH, D_SURFACE_EPOCH, D_SHADOW_LIST, D_CAMERA_LIST,
    D_N_WORK_SHADOW, D_N_WORK_CAMERA, D_COPY_GEN, D_COPY_OVERLAY, D_COPY_IDS_WAIT,
    D_SMAP_VALID, D_SMAP_AGE, D_CAM_PREV_VALID, D_R2_SETTLED, D_PLAN_VALID, D_PLAN_TWO_ROUND, D_VIS_HISTORY, D_LIST_VALID_SHADOW, D_LIST_VALID_CAMERA,
    D_PLAN_BEHIND_CAM, D_GBUF_LANE, D_SFLAG_HISTORY, D_COUNT
};
static const int kValues[D_COUNT] = { 2, 2, 2, 2, 2, 4, 2, 2, 2, 3,  2, 4, 2, 2, 2, 2, 2, 3, 3,  2, 2, 4, 4, 4,  2, 2, 2, 2, 2, 2, 2, 2, 2,  2, 3, 2 };

static void flag(Case& c, uint32_t bit, int v) { c.f.flags = v ? c.f.flags | bit : c.f.flags & ~bit; }
// a pass's work list: 0 none, 1 built from this frame's block, 2 built from another
static void list(Case& c, int slot, int v) { c.f.use_worklist[slot] = v != 0; c.f.block_is_list[slot] = v == 1; }

// (D_FRAME_NO comes before D_SMAP_AGE in every sweep: the map's age is counted back from the frame)
static void set(Case& c, Dim d, int v)
{
    switch (d) {
    case D_NO_HIZ: flag(c, ZRP_NO_HIZ, v); break;
    case D_SERIAL: flag(c, ZRP_SERIAL_PASSES, v); break;
    case D_NO_LIST_REUSE: flag(c, ZRP_NO_LIST_REUSE, v); break;
    case D_SHADOW_OCCLUSION: flag(c, ZRP_SHADOW_OCCLUSION, v); break;
    case D_NO_SHADOW_OCCLUSION: flag(c, ZRP_NO_SHADOW_OCCLUSION, v); break;
    case D_PARTITION: c.f.tile_world = v == 1 ? 2 : 1; c.f.shadow_world = v == 2 ? 2 : 1; c.f.stile_world = v == 3 ? 2 : 1; break;
    case D_MAP_EXTERNAL: c.f.map_external = v != 0; break;
    case D_SKY: c.f.sky = v != 0; break;
    case D_FORWARD: c.f.shading = v ? ZRP_SHADING_FORWARD : 0u; break;
    case D_ENTRY: c.f.entry = (ZrEntry)v; break;
    case D_HAS_LANE: c.f.has_lane = v != 0; break;
    case D_FRAME_NO: c.f.frame_no = (uint64_t)v; break;
    case D_SHADOW_IS_MAP: c.f.shadow_is_map = v != 0; break;
    case D_CAMERA_IS_PREV: c.f.camera_is_prev = v != 0; break;
    case D_CASTER_EPOCH: c.f.caster_epoch = c.k.smap_epoch + (v ? 0u : 1u); break;
    case D_CAMERA_EPOCH: c.f.camera_epoch = c.k.cam_prev_epoch + (v ? 0u : 1u); break;
    case D_SURFACE_EPOCH: c.f.surface_epoch = c.k.surf_prev_epoch + (v ? 0u : 1u); break;
    case D_SHADOW_LIST: list(c, 0, v); break;
    case D_CAMERA_LIST: list(c, 1, v); break;
    case D_N_WORK_SHADOW: c.f.n_work[0] = v ? 100000u : 0u; break;      // (100 000: more than one per five texels of a 256^2 map)
    case D_N_WORK_CAMERA: c.f.n_work[1] = v ? 1000u : 0u; break;
    case D_COPY_GEN: c.f.copy_gen[0] = (v & 1) ? 5 : 4; c.f.copy_gen[1] = (v & 2) ? 5 : 4; break;      // (bit i clear: copy i is of an earlier run)
    case D_COPY_OVERLAY: c.f.copy_overlay[0] = (v & 1) != 0; c.f.copy_overlay[1] = (v & 2) != 0; break;
    case D_COPY_IDS_WAIT: c.f.copy_ids_wait[0] = (v & 1) != 0; c.f.copy_ids_wait[1] = (v & 2) != 0; break;
    case D_SMAP_VALID: c.k.smap_valid = v != 0; break;
    case D_SMAP_AGE: c.k.smap_frame = v ? (c.f.frame_no >= 2 ? c.f.frame_no - 2 : 0) : (c.f.frame_no >= 1 ? c.f.frame_no - 1 : 0); break;
    case D_CAM_PREV_VALID: c.k.cam_prev_valid = v != 0; break;
    case D_R2_SETTLED: c.k.r2_settled = v != 0; break;
    case D_PLAN_VALID: c.k.plan_valid = v != 0; break;
    case D_PLAN_TWO_ROUND: c.k.plan_two_round = v != 0; break;
    case D_VIS_HISTORY: c.k.vis_history = v != 0; break;
    case D_LIST_VALID_SHADOW: c.k.list_valid[0] = v != 0; break;
    case D_LIST_VALID_CAMERA: c.k.list_valid[1] = v != 0; break;
    case D_PLAN_BEHIND_CAM: c.k.plan_behind_cam = v != 0; break;
    case D_GBUF_LANE: c.k.gbuf_lane = (ZrLane)v; break;
    case D_SFLAG_HISTORY: c.k.sflag_history = v != 0; break;
    default: break;
    }
}

static int g_broken = 0;
static unsigned long long g_seen[5] = { 0, 0, 0, 0, 0 };      // plans that kept the map / kept the camera pass whole / deferred the resolve / had their head on the lane / kept round 2

#define HOLDS(cond) do { if (!(cond)) { if (g_broken++ < 20) printf("broken: %s (line %d) flags=%u entry=%d frame=%llu\n", #cond, __LINE__, f.flags, (int)f.entry, (unsigned long long)f.frame_no); } } while (0)
#define IMPLIES(a, b) HOLDS(!(a) || (b))

static void check(const Case& c)
{
    const ZrFrameFacts& f = c.f; const ZrFrameCarry& k = c.k;
    const ZrFramePlan p = zr_frame_plan(f, k);
    const bool lanes = f.has_lane && !(f.flags & ZRP_SERIAL_PASSES) && f.entry != ZR_ENTRY_STAGED;
    const bool head_on_lane = p.camera_keep && p.head == ZR_LANE_CAM;
    g_seen[0] += p.shadow_keep; g_seen[1] += p.camera_keep; g_seen[2] += p.resolve_deferred; g_seen[3] += head_on_lane; g_seen[4] += p.rounds == ZR_ROUNDS_TWO_KEPT;
    // a kept shadow map: an unpartitioned context's own map, and neither flag
    IMPLIES(p.shadow_keep, f.tile_world <= 1 && f.shadow_world <= 1 && f.stile_world <= 1 && !f.map_external &&
                           !(f.flags & (ZRP_NO_LIST_REUSE | ZRP_SHADOW_OCCLUSION)));
    IMPLIES(p.shadow_keep, k.smap_valid && k.smap_epoch == f.caster_epoch && f.shadow_is_map);
    HOLDS(p.shadow_keep == (p.shadow == ZR_LANE_NONE));
    IMPLIES(p.shadow_keep, !p.shadow_occlusion);
    // the camera pass kept whole
    IMPLIES(p.camera_keep, p.rounds == ZR_ROUNDS_TWO_KEPT && !p.camera_list_rebuild && k.plan_valid && k.vis_history && f.n_work[1] != 0 &&
                           !(f.flags & ZRP_NO_HIZ) && !f.sky);
    IMPLIES(p.camera_keep, f.copy_gen[0] == p.g_gen && f.copy_gen[1] == p.g_gen && !f.copy_overlay[0] && !f.copy_overlay[1]);
    IMPLIES(p.camera_keep, p.camera == ZR_LANE_NONE && p.resolve == ZR_LANE_NONE && !p.resolve_deferred && !p.reset_stats && !p.reset_camera_list &&
                           (p.ev_cam == ZR_EVCAM_NONE || p.ev_cam == ZR_EVCAM_BEHIND_ONE_PIXEL) && !p.wait_lane_end && !p.wait_ids && !p.ids_taken);
    HOLDS(p.camera_keep == (p.camera == ZR_LANE_NONE) && p.camera_keep == (p.resolve == ZR_LANE_NONE));
    IMPLIES(p.rounds == ZR_ROUNDS_TWO_KEPT, !(f.flags & ZRP_NO_LIST_REUSE) && k.cam_prev_valid && k.r2_settled && k.cam_prev_epoch == f.camera_epoch && f.camera_is_prev);
    // the resolve on the host's stream beside a camera pipeline on the lane
    IMPLIES(p.resolve_deferred, f.entry == ZR_ENTRY_RENDER && lanes && p.shadow_keep && !p.camera_keep && !f.sky);
    HOLDS(p.resolve_deferred == (p.resolve == ZR_LANE_HOST && p.camera == ZR_LANE_CAM));
    IMPLIES(!p.camera_keep && !p.resolve_deferred, p.resolve == p.camera);
    // the head of a kept frame on the lane
    IMPLIES(head_on_lane, p.shadow_keep && lanes && f.entry == ZR_ENTRY_RENDER && k.smap_frame + 2 <= f.frame_no && p.one_pixel != ZR_LANE_HOST);
    IMPLIES(!p.camera_keep, p.head == p.camera);
    IMPLIES(p.one_pixel == ZR_LANE_CAM, head_on_lane);
    // ev_cam: one place at most (it is one value), on the lane, and the host's stream waits for it exactly then
    const bool on_lane = p.head == ZR_LANE_CAM || p.camera == ZR_LANE_CAM || p.one_pixel == ZR_LANE_CAM;
    HOLDS((p.ev_cam != ZR_EVCAM_NONE) == on_lane && p.host_waits_ev_cam == on_lane);
    IMPLIES(p.ev_cam == ZR_EVCAM_BEHIND_MARK, p.resolve_deferred);
    IMPLIES(p.ev_cam == ZR_EVCAM_BEHIND_ONE_PIXEL, head_on_lane);
    IMPLIES(p.ev_cam == ZR_EVCAM_LANE_END || p.ev_cam == ZR_EVCAM_BEHIND_RESOLVE, p.camera == ZR_LANE_CAM && p.resolve == ZR_LANE_CAM);
    // staged entry points and serial contexts: one stream
    IMPLIES(!lanes, p.head == ZR_LANE_HOST && p.shadow != ZR_LANE_CAM && p.camera != ZR_LANE_CAM && p.resolve != ZR_LANE_CAM && p.one_pixel != ZR_LANE_CAM &&
                    p.ev_cam == ZR_EVCAM_NONE && !p.host_waits_ev_cam && !p.wait_end2 && !p.wait_end1 && !p.wait_ids && p.ev_join);
    HOLDS(p.lighting == ZR_LANE_HOST && p.shadow != ZR_LANE_CAM);
    // the waits
    HOLDS(p.wait_end2 == (p.head == ZR_LANE_CAM && f.frame_no >= 2));
    IMPLIES(p.wait_end1, p.head == ZR_LANE_CAM && k.gbuf_lane == ZR_LANE_HOST && f.frame_no >= 1);
    IMPLIES(p.wait_lane_end, p.head == ZR_LANE_HOST && k.plan_behind_cam && p.camera == ZR_LANE_HOST);
    IMPLIES(k.plan_behind_cam && p.camera == ZR_LANE_HOST && f.has_lane, p.wait_lane_end);
    IMPLIES(p.wait_ids, p.ids_taken && p.head == ZR_LANE_CAM);
    // the rounds
    IMPLIES(p.count_first, p.rounds != ZR_ROUNDS_TWO_KEPT);
    HOLDS((p.rounds == ZR_ROUNDS_ONE) == !(p.hiz_on && k.vis_history) && (int)ZR_ROUNDS_ONE == 0);
    IMPLIES(!k.plan_valid && !p.camera_keep, p.count_first);
    // Nothing is kept that was not completely enqueued: were the frame to fail behind its head, the same frame planned again would draw what
    // this one meant to draw and rebuild what it meant to rebuild.
    const ZrFrameCarry failed = zr_frame_carry(k, f, p, ZR_STAGE_HEAD);
    ZrFrameFacts again = f; again.block_is_list[0] = again.block_is_list[1] = true;      // (the keys are this frame's blocks by then)
    const ZrFramePlan q = zr_frame_plan(again, failed);
    IMPLIES(!p.shadow_keep, !q.shadow_keep);
    IMPLIES(!p.camera_keep, !q.camera_keep && q.rounds != ZR_ROUNDS_TWO_KEPT);
    IMPLIES(p.shadow_list_rebuild, q.shadow_list_rebuild);
    IMPLIES(p.camera_list_rebuild, q.camera_list_rebuild);
    // ... and a frame that went through leaves what its stages made
    ZrFrameCarry done = failed;
    if (p.shadow != ZR_LANE_NONE) done = zr_frame_carry(done, f, p, ZR_STAGE_SHADOW);
    if (p.camera != ZR_LANE_NONE) done = zr_frame_carry(done, f, p, ZR_STAGE_CAMERA);
    HOLDS(done.smap_valid && done.g_gen == p.g_gen && done.surf_prev_epoch == f.surface_epoch);
    IMPLIES(p.shadow != ZR_LANE_NONE, done.smap_epoch == f.caster_epoch && done.smap_frame == f.frame_no);
    IMPLIES(p.camera != ZR_LANE_NONE, done.gbuf_lane == p.camera && done.cam_prev_valid == p.hiz_on && done.vis_history == p.hiz_on && done.cam_prev_epoch == f.camera_epoch &&
                                      done.plan_behind_cam == (p.ev_cam == ZR_EVCAM_BEHIND_MARK || p.ev_cam == ZR_EVCAM_BEHIND_RESOLVE));
    IMPLIES(p.camera_keep, done.plan_behind_cam == k.plan_behind_cam && done.gbuf_lane == k.gbuf_lane && done.r2_settled && done.cam_prev_valid);
}

static unsigned long long sweep(const char* name, const Dim* dims, int n)
{
    int v[D_COUNT] = { 0 };
    unsigned long long visited = 0;
    for (;;) {
        Case c = resting();
        for (int i = 0; i < n; ++i) set(c, dims[i], v[i]);
        check(c);
        ++visited;
        int i = 0;
        while (i < n && ++v[i] == kValues[dims[i]]) v[i++] = 0;
        if (i == n) break;
    }
    printf("swept %s %llu\n", name, visited);
    return visited;
}

int main()
{
    sequences();
    static const Dim shadow[] = { D_NO_LIST_REUSE, D_SHADOW_OCCLUSION, D_NO_SHADOW_OCCLUSION, D_PARTITION, D_MAP_EXTERNAL, D_SERIAL, D_ENTRY, D_HAS_LANE,
                                  D_FRAME_NO, D_SHADOW_IS_MAP, D_CASTER_EPOCH, D_SHADOW_LIST, D_N_WORK_SHADOW, D_SMAP_VALID, D_SMAP_AGE, D_LIST_VALID_SHADOW, D_SFLAG_HISTORY };
    static const Dim camera[] = { D_NO_HIZ, D_NO_LIST_REUSE, D_SKY, D_CAMERA_IS_PREV, D_CAMERA_EPOCH, D_SURFACE_EPOCH, D_CAMERA_LIST, D_N_WORK_CAMERA,
                                  D_COPY_GEN, D_COPY_OVERLAY, D_SMAP_VALID, D_CAM_PREV_VALID, D_R2_SETTLED, D_PLAN_VALID, D_PLAN_TWO_ROUND, D_VIS_HISTORY, D_LIST_VALID_CAMERA };
    static const Dim lanes[] = { D_SERIAL, D_SKY, D_FORWARD, D_ENTRY, D_HAS_LANE, D_FRAME_NO, D_COPY_GEN, D_COPY_IDS_WAIT,
                                 D_SMAP_VALID, D_SMAP_AGE, D_R2_SETTLED, D_PLAN_VALID, D_VIS_HISTORY, D_PLAN_BEHIND_CAM, D_GBUF_LANE };
    unsigned long long total = 0;
    total += sweep("shadow", shadow, (int)(sizeof shadow / sizeof *shadow));
    total += sweep("camera", camera, (int)(sizeof camera / sizeof *camera));
    total += sweep("lanes", lanes, (int)(sizeof lanes / sizeof *lanes));
    printf("swept all %llu\n", total);
    printf("seen map_kept=%llu camera_whole=%llu resolve_deferred=%llu head_on_lane=%llu round2_kept=%llu\n", g_seen[0], g_seen[1], g_seen[2], g_seen[3], g_seen[4]);
    printf("broken %d\n", g_broken);
    return g_broken ? 1 : 0;
}
