// lighting_keep_plan_check.cpp — the lighting pass's keep (csrc/zr_frame_plan.h: ZrFramePlan::light_keep / light_fill, ZR_STAGE_LIGHTING) run
// without a GPU, over that header alone, as frame_plan_check.cpp runs the rest of the schedule: tests/test_lighting_keep_plan.py compiles
// this file, runs it and holds what it prints against expectations written out there.
//
// Scripted sequences of frames through zr_frame_plan / zr_frame_carry as frame_begin, shadow_pass, gbuffer_pass and lighting_pass drive
// them: "== <name>", then per frame "frame=<n> map=<kept|drawn> pass=<whole|drawn> light=<ignored|filled|read>".
#include "zr_frame_plan.h"

#include <cstdio>

// What zr_ctx holds beside the carry, reduced to what the facts are made from: pass blocks and standing uniforms as numbers.
struct Host {
    ZrFrameFacts f;
    ZrFrameCarry k;
    int shadow_block = 1, camera_block = 1, uniforms = 1;      // this frame's
    int smap_key = 0, cam_prev_key = 0, list_key[2] = { 0, 0 }, light_key = 0;
    bool plane = false, no_room = false;                       // the plane exists / can never be made
    uint64_t frame_no = 0, copy_gen[2] = { 0, 0 };
};

static Host host(ZrEntry entry, bool has_lane, uint32_t flags = 0)
{
    Host h;
    h.f.flags = flags; h.f.SD = 256; h.f.n_work[0] = h.f.n_work[1] = 1000; h.f.entry = entry; h.f.has_lane = has_lane;
    h.f.cube_gen = 1;
    return h;
}

static void frame(Host& h)
{
    ZrFrameFacts& f = h.f;
    f.frame_no = h.frame_no;
    f.shadow_is_map = h.smap_key == h.shadow_block; f.camera_is_prev = h.cam_prev_key == h.camera_block;
    f.block_is_list[0] = h.list_key[0] == h.shadow_block; f.block_is_list[1] = h.list_key[1] == h.camera_block;
    for (int i = 0; i < 2; ++i) f.copy_gen[i] = h.copy_gen[i];
    f.light_plane_ok = !h.no_room; f.light_uniforms_same = h.plane && h.light_key == h.uniforms;      // (zr_light_facts)
    ZrFramePlan p = zr_frame_plan(f, h.k);
    if (p.light_fill && !h.plane) {                                // (zr_light_plane_make, and the second plan where it fails)
        if (h.no_room) { f.light_plane_ok = false; p = zr_frame_plan(f, h.k); }
        else h.plane = true;
    }
    h.k = zr_frame_carry(h.k, f, p, ZR_STAGE_HEAD);
    if (p.shadow_list_rebuild) h.list_key[0] = h.shadow_block;
    if (p.camera_list_rebuild) h.list_key[1] = h.camera_block;
    if (p.shadow != ZR_LANE_NONE) { h.smap_key = h.shadow_block; h.k = zr_frame_carry(h.k, f, p, ZR_STAGE_SHADOW); }
    if (p.camera != ZR_LANE_NONE) {
        h.copy_gen[h.frame_no & 1u] = p.g_gen;
        h.cam_prev_key = h.camera_block; h.k = zr_frame_carry(h.k, f, p, ZR_STAGE_CAMERA);
    }
    if (p.light_fill) { h.light_key = h.uniforms; h.k = zr_frame_carry(h.k, f, p, ZR_STAGE_LIGHTING); }
    printf("frame=%llu map=%s pass=%s light=%s lighting=%s both=%d\n", (unsigned long long)h.frame_no, p.shadow_keep ? "kept" : "drawn",
           p.camera_keep ? "whole" : "drawn", p.light_keep ? "read" : p.light_fill ? "filled" : "ignored",
           p.lighting == ZR_LANE_HOST ? "host" : "other", (int)(p.light_keep && p.light_fill));
    h.frame_no++;
}

static void frames(Host& h, int n) { for (int i = 0; i < n; ++i) frame(h); }

int main()
{
    const struct { const char* name; ZrEntry entry; bool lane; uint32_t flags; } rests[] = {
        { "rest_render", ZR_ENTRY_RENDER, true, 0u }, { "rest_serial", ZR_ENTRY_RENDER, true, ZRP_SERIAL_PASSES },
        { "rest_staged", ZR_ENTRY_STAGED, true, 0u }, { "rest_geometry", ZR_ENTRY_GEOMETRY, true, 0u },
        { "no_list_reuse", ZR_ENTRY_RENDER, true, ZRP_NO_LIST_REUSE } };
    for (const auto& r : rests) { printf("== %s\n", r.name); Host h = host(r.entry, r.lane, r.flags); frames(h, 6); }

    // each of (a) - (e) failing alone: four resting frames (drawn, drawn, filled, read), the change, five more
    { printf("== a_camera_moves\n"); Host h = host(ZR_ENTRY_RENDER, true); frames(h, 4); h.camera_block = 2; frames(h, 5); }
    { printf("== a_surface_changes\n"); Host h = host(ZR_ENTRY_RENDER, true); frames(h, 4); h.f.surface_epoch++; frames(h, 5); }
    { printf("== b_light_moves\n"); Host h = host(ZR_ENTRY_RENDER, true); frames(h, 4); h.shadow_block = 2; frames(h, 5); }
    { printf("== b_casters_change\n"); Host h = host(ZR_ENTRY_RENDER, true); frames(h, 4); h.f.caster_epoch++; frames(h, 5); }
    { printf("== b_map_external\n"); Host h = host(ZR_ENTRY_RENDER, true); frames(h, 4); h.f.map_external = true; h.f.caster_epoch++; frames(h, 3);
      h.f.map_external = false; h.f.caster_epoch++; frames(h, 4); }
    { printf("== c_uniforms_change\n"); Host h = host(ZR_ENTRY_RENDER, true); frames(h, 4); h.uniforms = 2; frames(h, 3); h.uniforms = 1; frames(h, 2); }
    { printf("== d_cubemap_replaced\n"); Host h = host(ZR_ENTRY_RENDER, true); frames(h, 4); h.f.cube_gen++; frames(h, 3); }
    { printf("== e_forward_and_back\n"); Host h = host(ZR_ENTRY_RENDER, true); frames(h, 4); h.f.shading = ZRP_SHADING_FORWARD; h.f.surface_epoch++; frames(h, 4);
      h.f.shading = 0; h.f.surface_epoch++; frames(h, 4); }
    // the empty-pixel shortcut goes off (debug view 6) and on again: one more fill, of every pixel, serves both
    { printf("== shortcut_off_and_on\n"); Host h = host(ZR_ENTRY_RENDER, true); frames(h, 4); h.f.light_empty_px = false; frames(h, 2);
      h.f.light_empty_px = true; frames(h, 2); h.f.light_empty_px = false; frames(h, 1); }
    // partitioned contexts draw their map every frame: nothing to keep it against
    { printf("== tile_world_2\n"); Host h = host(ZR_ENTRY_RENDER, true); h.f.tile_world = 2; frames(h, 6); }
    { printf("== shadow_world_2\n"); Host h = host(ZR_ENTRY_STAGED, true); h.f.shadow_world = 2; frames(h, 6); }
    { printf("== stile_world_4\n"); Host h = host(ZR_ENTRY_STAGED, true); h.f.stile_world = 4; frames(h, 6); }
    // a context that never asked, one without room for the plane
    { printf("== no_room\n"); Host h = host(ZR_ENTRY_RENDER, true); h.no_room = true; frames(h, 6); }
    // the carry starts over (every number in it counts from its first value again): the plane must not match by number
    { printf("== carry_reset\n"); Host h = host(ZR_ENTRY_RENDER, true); frames(h, 4);
      h.k = ZrFrameCarry(); h.smap_key = h.cam_prev_key = h.list_key[0] = h.list_key[1] = 0; h.copy_gen[0] = h.copy_gen[1] = 0; h.frame_no = 0; frames(h, 4); }
    // the stream changed (zr_history_forgotten's bit for the plane, with the casters' epoch)
    { printf("== plane_forgotten\n"); Host h = host(ZR_ENTRY_RENDER, true); frames(h, 4); h.k.light_valid = false; frames(h, 2); }
    return 0;
}
