// rest_plan_check.cpp — the one-launch resting frame in the schedule (csrc/zr_frame_plan.h: ZrFrameFacts::light_by_arg,
// ZrFramePlan::light_args) run without a GPU: tests/test_rest_plan.py compiles this file, runs it and holds what it prints against
// expectations written out there.
//
// frame_plan_check.cpp is compiled into this program as it stands - its sequences, its three sweeps, every invariant of its check() -
// with zr_frame_plan() replaced by a wrapper that gives each frame a context whose lighting pass keeps: the plane can be made, the
// standing uniforms are the fill's, and light_by_arg is off (first run) or on (second run).  In the sweeps the carry says the plane was
// filled from the very run of GBuffer copies and the very map the resting frame reads; in the sequences the wrapper carries what
// lighting_pass carries (ZR_STAGE_LIGHTING) from frame to frame.  On top of check()'s invariants, for every plan made:
//   light_args implies light_keep, one_pixel == NONE, head == HOST and no event or wait at the head;
//   light_args never holds on a frame that fills or draws anything;  light_args only where the fact allows it;
//   a frame that fills, in a context that has the slot, has its head - the one-pixel launch that writes the slot - on the host's stream.
// Output: frame_plan_check's own, twice, each run behind a line "rest by_arg=<0|1>"; then "rest_seen ..." and "rest_broken <n>".
#include "zr_frame_plan.h"

#include <cstdio>

static bool g_by_arg = false, g_sequence = false, g_slot = true;      // (g_slot: the context has the slot; off for one sequence)
static int g_rest_broken = 0;
static unsigned long long g_rest_seen[3] = { 0, 0, 0 };      // plans with light_args / light_keep / light_fill
static struct { bool valid; uint64_t g_gen, smap_frame; } g_light = { false, 0, 0 };      // what the last fill of a sequence left

#define REST_HOLDS(cond) do { if (!(cond)) { if (g_rest_broken++ < 20) printf("rest broken: %s (line %d) flags=%u entry=%d frame=%llu\n", #cond, __LINE__, f.flags, (int)f.entry, (unsigned long long)f.frame_no); } } while (0)
#define REST_IMPLIES(a, b) REST_HOLDS(!(a) || (b))

static ZrFramePlan rest_plan(const ZrFrameFacts& f0, const ZrFrameCarry& k0)
{
    ZrFrameFacts f = f0; ZrFrameCarry k = k0;
    f.light_plane_ok = true; f.light_uniforms_same = true; f.light_empty_px = true; f.light_by_arg = g_by_arg; f.light_slot = g_slot; f.cube_gen = 1;
    k.light_cube_gen = 1; k.light_all_px = false;
    if (g_sequence) { k.light_valid = g_light.valid; k.light_g_gen = g_light.g_gen; k.light_smap_frame = g_light.smap_frame; }
    else { k.light_valid = true; k.light_g_gen = k.g_gen; k.light_smap_frame = k.smap_frame; }
    const ZrFramePlan p = zr_frame_plan(f, k);
    g_rest_seen[0] += p.light_args; g_rest_seen[1] += p.light_keep; g_rest_seen[2] += p.light_fill;
    REST_IMPLIES(p.light_args, p.light_keep && p.one_pixel == ZR_LANE_NONE && p.head == ZR_LANE_HOST && p.ev_cam == ZR_EVCAM_NONE && !p.host_waits_ev_cam &&
                               !p.wait_end2 && !p.wait_end1 && !p.wait_lane_end && !p.wait_ids);
    REST_IMPLIES(p.light_args, !p.light_fill && p.shadow == ZR_LANE_NONE && p.camera == ZR_LANE_NONE && p.resolve == ZR_LANE_NONE && p.shadow_keep && p.camera_keep &&
                               !p.reset_stats && !p.reset_camera_list);
    REST_IMPLIES(p.light_args, f.light_by_arg && f.shading != ZRP_SHADING_FORWARD && !(f.flags & ZRP_NO_LIST_REUSE));
    REST_HOLDS(p.light_args == (p.light_keep && f.light_by_arg));
    REST_HOLDS(!(p.light_keep && p.light_fill));
    REST_IMPLIES(p.light_fill && f.light_slot, p.head == ZR_LANE_HOST && p.one_pixel != ZR_LANE_CAM);
    REST_IMPLIES(f.light_by_arg, f.light_slot);      // (as zr_light_facts makes them)
    REST_IMPLIES(p.light_keep || p.light_fill, p.lighting == ZR_LANE_HOST);
    if (g_sequence && p.light_fill) { g_light.valid = true; g_light.g_gen = p.g_gen; g_light.smap_frame = k.smap_frame; }
    return p;
}

#define zr_frame_plan rest_plan
#define main frame_plan_check_main
#include "frame_plan_check.cpp"
#undef main
#undef zr_frame_plan

// frame_plan_check's sequences make one plan per frame; its sweeps plan a case three times (the frame, the frame planned again after a
// failure, ...), which must not carry anything over: the wrapper carries the fill only while the sequences run.
int main()
{
    for (int by_arg = 0; by_arg < 2; ++by_arg) {
        g_by_arg = by_arg != 0;
        printf("rest by_arg=%d\n", by_arg);
        g_sequence = true; g_light.valid = false;
        puts("== rest_render"); { Host h = host(ZR_ENTRY_RENDER, true); for (int i = 0; i < 8; ++i) frame(h); }
        g_light.valid = false;
        puts("== rest_staged"); { Host h = host(ZR_ENTRY_STAGED, true); for (int i = 0; i < 8; ++i) frame(h); }
        g_light.valid = false;
        puts("== light_stops"); { Host h = host(ZR_ENTRY_RENDER, true); for (int i = 0; i < 8; ++i) { if (i <= 4) h.shadow_block = 10 + i; frame(h); } }
        if (!by_arg)      // the plane is forgotten in the middle of a rest (frame 5 fills again): with the slot, and in a context without it
            for (int slot = 1; slot >= 0; --slot) {
                g_light.valid = false; g_slot = slot != 0;
                puts(slot ? "== refill_slot" : "== refill_no_slot");
                Host h = host(ZR_ENTRY_RENDER, true);
                for (int i = 0; i < 8; ++i) { if (i == 5) g_light.valid = false; frame(h); }
                g_slot = true;
            }
        g_sequence = false;
        static const Dim shadow[] = { D_NO_LIST_REUSE, D_SHADOW_OCCLUSION, D_NO_SHADOW_OCCLUSION, D_PARTITION, D_MAP_EXTERNAL, D_SERIAL, D_ENTRY, D_HAS_LANE,
                                      D_FRAME_NO, D_SHADOW_IS_MAP, D_CASTER_EPOCH, D_SHADOW_LIST, D_N_WORK_SHADOW, D_SMAP_VALID, D_SMAP_AGE, D_LIST_VALID_SHADOW, D_SFLAG_HISTORY };
        static const Dim camera[] = { D_NO_HIZ, D_NO_LIST_REUSE, D_SKY, D_CAMERA_IS_PREV, D_CAMERA_EPOCH, D_SURFACE_EPOCH, D_CAMERA_LIST, D_N_WORK_CAMERA,
                                      D_COPY_GEN, D_COPY_OVERLAY, D_SMAP_VALID, D_CAM_PREV_VALID, D_R2_SETTLED, D_PLAN_VALID, D_PLAN_TWO_ROUND, D_VIS_HISTORY, D_LIST_VALID_CAMERA };
        static const Dim lanes[] = { D_SERIAL, D_SKY, D_FORWARD, D_ENTRY, D_HAS_LANE, D_FRAME_NO, D_COPY_GEN, D_COPY_IDS_WAIT,
                                     D_SMAP_VALID, D_SMAP_AGE, D_R2_SETTLED, D_PLAN_VALID, D_VIS_HISTORY, D_PLAN_BEHIND_CAM, D_GBUF_LANE };
        sweep("shadow", shadow, (int)(sizeof shadow / sizeof *shadow));
        sweep("camera", camera, (int)(sizeof camera / sizeof *camera));
        sweep("lanes", lanes, (int)(sizeof lanes / sizeof *lanes));
        printf("broken %d\n", g_broken);
    }
    printf("rest_seen light_args=%llu light_keep=%llu light_fill=%llu\n", g_rest_seen[0], g_rest_seen[1], g_rest_seen[2]);
    printf("rest_broken %d\n", g_rest_broken);
    (void)&frame_plan_check_main;
    return g_broken || g_rest_broken ? 1 : 0;
}
