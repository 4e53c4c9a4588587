// zr_frame_plan.h — the frame schedule as a function ("The schedule"): what a frame keeps of the frames before it,
// which stream each of its stages runs on, and where the two lanes meet.  zr_frame_plan() decides a frame once, from values; the passes
// of zr_frame_host.cpp only read the plan.  zr_frame_carry() is the other half: what a finished stage leaves for the frames behind it.
// Plain C++17 and nothing of HIP: tests/frame_plan_check.cpp compiles this header alone and runs the schedule without a GPU.
#pragma once

#include <cstdint>

// Two schedule constants, re-measured whenever the balance of the two lanes changes (tools/ab_schedule.sh builds the variants; the others:
// zr_context.cpp): whether a zr_render frame that draws its shadow map records ev_cam ahead of its k_plan too (a frame that resolves on
// the host's stream always does) ...
#ifndef ZR_EV_CAM_AHEAD_OF_PLAN
#define ZR_EV_CAM_AHEAD_OF_PLAN 0
#endif
// ... and where the head of a zr_render frame that keeps camera pass and shadow map runs - the uniform upload and the one-pixel launch, some
// 15 us of latency ahead of k_lighting: 0 in series on the host's stream, 1 on the idle camera lane beside the previous frame's lighting
// pass, at the price of one event crossing (DESIGN.md section 7 has both, measured: 17 470 / 19 240 Mpixel/s).
#ifndef ZR_KEPT_HEAD_ON_LANE
#define ZR_KEPT_HEAD_ON_LANE 1
#endif
constexpr bool kZrEvCamAheadOfPlan = ZR_EV_CAM_AHEAD_OF_PLAN != 0, kZrKeptHeadOnLane = ZR_KEPT_HEAD_ON_LANE != 0;

// The zr_config flags the schedule reads, the shading mode that has no one-pixel launch and what k_plan is told about the rounds, under
// names of this header's own (zelda_render.h and zr_types.h have the originals; zr_frame_host.cpp asserts that they agree).
enum : uint32_t { ZRP_NO_HIZ = 8u, ZRP_SERIAL_PASSES = 16u, ZRP_NO_LIST_REUSE = 256u, ZRP_NO_SHADOW_OCCLUSION = 512u, ZRP_SHADOW_OCCLUSION = 1024u,
                  ZRP_SHADING_FORWARD = 1u };
enum ZrRounds : uint8_t { ZR_ROUNDS_ONE = 0, ZR_ROUNDS_TWO = 1, ZR_ROUNDS_TWO_KEPT = 2 };      // = ZR_PLAN_ONE_ROUND, _DREW_ROUND2, _KEPT_ROUND2

enum ZrLane : uint8_t { ZR_LANE_NONE, ZR_LANE_HOST, ZR_LANE_CAM };      // not run / the host's stream / the library's camera lane (cam_s)
// Who begins the frame: zr_render (all of it), zr_render_geometry (both geometry passes; the host lights it later) or zr_render_shadow
// (the staged entry points: one stream, a host's collectives between the stages).
enum ZrEntry : uint8_t { ZR_ENTRY_RENDER, ZR_ENTRY_GEOMETRY, ZR_ENTRY_STAGED };
// Where the frame records ev_cam, the one event the host's stream waits for before it lights the frame.
enum ZrEvCam : uint8_t {
    ZR_EVCAM_NONE,                  // nothing of the frame runs on the lane
    ZR_EVCAM_BEHIND_MARK,           // a resolve on the host's stream: behind k_mark, ahead of k_plan
    ZR_EVCAM_BEHIND_RESOLVE,        // ZR_EV_CAM_AHEAD_OF_PLAN builds: behind the lane's resolve, ahead of k_plan
    ZR_EVCAM_BEHIND_ONE_PIXEL,      // a kept frame's head on the lane: behind upload and one-pixel launch
    ZR_EVCAM_LANE_END               // behind the whole camera pipeline, k_plan included
};
enum ZrStage : uint8_t { ZR_STAGE_HEAD, ZR_STAGE_SHADOW, ZR_STAGE_CAMERA, ZR_STAGE_LIGHTING };      // the stages that leave something in the carry

// Everything the decision reads, as values (frame_begin gathers them once the frame's two pass blocks are built).
struct ZrFrameFacts {
    // the context's standing properties
    uint32_t flags = 0, tile_world = 1, shadow_world = 1, stile_world = 1;      // zr_config::flags; the frame's / the casters' / the map's partition
    bool map_external = false;             // the map is the caller's buffer (zr_set_shadow_buffer)
    bool sky = false;                      // a skydome is drawn (sky_set && sky_enabled)
    uint32_t shading = 0, SD = 0;          // ZR_SHADING_*; the map's edge
    uint32_t n_work[2] = { 0, 0 };         // meshlet-instances per pass (0 shadow, 1 camera; 0: the pass is its clear)
    bool use_worklist[2] = { false, false };      // the pass goes through an instance-level work list
    // the call
    ZrEntry entry = ZR_ENTRY_RENDER;
    bool has_lane = false;                 // the library has a camera lane (cam_s)
    uint64_t frame_no = 0;
    // the three epochs as they stand now (zr_casters_changed, zr_camera_changed, zr_surface_changed)
    uint64_t caster_epoch = 0, camera_epoch = 0, surface_epoch = 0;
    // the pass blocks, compared by the caller: the shadow block is the one the current map was drawn from, the camera block is the
    // previous frame's, each pass's block is the one its work list on the device was built from
    bool shadow_is_map = false, camera_is_prev = false, block_is_list[2] = { false, false };
    // the two GBuffer copies (index: frame parity): the run of equal inputs each was last resolved in, skydome pixels left in its
    // overlay plane, a census enqueued against it that its next writer waits for
    uint64_t copy_gen[2] = { 0, 0 };
    bool copy_overlay[2] = { false, false }, copy_ids_wait[2] = { false, false };
    // The lighting pass's plane of standing terms (ZrFramePlan::light_keep).  light_plane_ok: the context can have one (false: it could
    // not be allocated - and every context that never asked).  light_uniforms_same: the standing uniforms, compared by the caller byte
    // for byte, are those of the fill.  cube_gen: the cubemap's contents (bumped whenever they are replaced).  light_empty_px: the frame's
    // lighting pass takes the empty-pixel shortcut (off: debug view 6, a diagnostic switch), and those pixels touch no plane.
    bool light_plane_ok = false, light_uniforms_same = false, light_empty_px = true;
    uint64_t cube_gen = 0;
    // A frame that reads the plane can be ONE launch (ZrFramePlan::light_args): at most ZR_REST_ARG_LIGHTS point lights, the empty-pixel
    // shortcut on, the fill's records and slot exist, and nothing behind the pass reads XkView (debug view 9 does).
    // light_slot: the context has (or, with its first fill, gets) the slot a fill's one-pixel launch writes for such frames.
    bool light_by_arg = false, light_slot = false;
};

// What the frames enqueued so far left behind, and nothing else.  (The ZrPass keys that go with it - smap_key, cam_prev_key, list_key[] -
// stay beside it in zr_ctx: the caller compares them, see ZrFrameFacts.)
struct ZrFrameCarry {
    // The shadow map of the last drawn pass: there is one, the caster epoch it was drawn at, the frame that drew it.
    bool smap_valid = false; uint64_t smap_epoch = 0, smap_frame = 0;
    // The camera pass of the frame enqueued last: it left a visibility history (cam_prev_valid) at this camera epoch; r2_settled: it drew
    // both rounds or kept round 2 AND its own inputs were its predecessor's, so the history its round 1 went by was the standing view's own.
    bool cam_prev_valid = false, r2_settled = false; uint64_t cam_prev_epoch = 0;
    // The record buckets' plan (k_plan): made at all / by a frame that drew two rounds.  vis_history: the visibility marks come from a
    // frame of this scene.  sflag_history: so do the shadow pass's occlusion flags (else: all set, and the first test takes every item).
    bool plan_valid = false, plan_two_round = false, vis_history = false, sflag_history = false;
    bool list_valid[2] = { false, false };      // the pass's work list on the device is the one of list_key[]
    // g_gen counts the runs of frames whose camera block and two epochs are the same (ZrFrameFacts::copy_gen: the run a copy was last
    // resolved in); surf_prev_epoch: the surface epoch of the frame enqueued last.
    uint64_t surf_prev_epoch = 0, g_gen = 1;
    // The last camera pipeline: the lane it ran on (NONE: there was none yet), and whether its ev_cam sat AHEAD of its k_plan - then a
    // camera pipeline on the host's stream waits for the lane's end first.
    ZrLane gbuf_lane = ZR_LANE_NONE; bool plan_behind_cam = false;
    // The lighting pass's plane: it holds the standing terms of a fill that was enqueued completely, and what that fill read - the run of
    // equal camera-pass inputs its GBuffer copy belonged to, the drawing frame of its shadow map, the cubemap's generation (its uniforms
    // stay beside the carry, like the pass blocks) - and whether it wrote every pixel (light_all_px: the shortcut was off).
    bool light_valid = false, light_all_px = false; uint64_t light_g_gen = 0, light_smap_frame = 0, light_cube_gen = 0;
};

// What this frame does.  Made once (frame_begin), read by every stage, changed by none.
struct ZrFramePlan {
    // per stage the lane, or NONE: the head (uniform upload + k_frame_begin), the shadow pipeline, the camera pipeline, the resolve,
    // the one-pixel launch, the lighting pass.  (Which timing events a frame records, and where: zr_timed.h.)
    ZrLane head = ZR_LANE_HOST, shadow = ZR_LANE_HOST, camera = ZR_LANE_HOST, resolve = ZR_LANE_HOST, one_pixel = ZR_LANE_HOST, lighting = ZR_LANE_HOST;
    // shadow pass: the map of the last drawn pass is kept / occlusion culling is on / the work list is rebuilt / reused
    bool shadow_keep = false, shadow_occlusion = false, shadow_list_rebuild = false, shadow_list_reuse = false;
    // camera pass: kept whole / the rounds (TWO_KEPT: the effective keep of round 2) / k_geom counts before round 1 draws / Hi-Z on /
    // the work list rebuilt / reused / the frame's inputs are the previous frame's / the run of equal inputs it belongs to
    bool camera_keep = false; ZrRounds rounds = ZR_ROUNDS_ONE;
    bool count_first = false, hiz_on = false, camera_list_rebuild = false, camera_list_reuse = false, cam_same = false;
    uint64_t g_gen = 1;
    bool resolve_deferred = false;         // the resolve is left to the lighting call, on the host's stream (the lane ends k_mark -> ev_cam -> k_plan)
    // head: k_frame_begin zeroes the camera lane's statistics / the camera list's length
    bool reset_stats = true, reset_camera_list = false;
    // waits at the head: for ev_end[N - 2] / ev_end[N - 1] (the lane changed) / the lane's end (ev_lane, recorded then) / a census (ev_ids);
    // ids_taken: the frame writes its copy, so a census pending against it is no longer waited for by anyone
    bool wait_end2 = false, wait_end1 = false, wait_lane_end = false, wait_ids = false, ids_taken = false;
    ZrEvCam ev_cam = ZR_EVCAM_NONE; bool host_waits_ev_cam = false;
    bool ev_join = false;                  // recorded behind the shadow stage (zr_stream_wait_shadow)
    // lighting pass: the standing terms of every pixel are read from the plane / computed as ever and stored into it (neither: the pass
    // ignores the plane)
    bool light_keep = false, light_fill = false;
    // light_args: a pass that reads the plane takes its moving uniforms as kernel arguments and computes the empty pixel's colour itself
    // (k_lighting_rest).  The frame is that one launch on the host's stream: no uniform upload, no one-pixel launch, no event, nothing on
    // the lane.  The device copy of XkView stays as stale as it was: the next frame that reads it uploads it.
    bool light_args = false;
};

static inline ZrFramePlan zr_frame_plan(const ZrFrameFacts& f, const ZrFrameCarry& k)
{
    ZrFramePlan p;
    // Two lanes: the camera pipeline on cam_s, the shadow pipeline and the lighting pass on the host's stream.  ZR_FLAG_SERIAL_PASSES
    // keeps everything on the one stream, as the staged entry points do.
    const bool lanes = f.has_lane && !(f.flags & ZRP_SERIAL_PASSES) && f.entry != ZR_ENTRY_STAGED;
    const bool render = f.entry == ZR_ENTRY_RENDER;

    // The work lists (k_cull_instances) are kept while the pass block and the scene stand still: rebuilt only when the block or the
    // scene changed (a list counts as standing only once its k_cull_instances has been enqueued: zr_frame_carry).
    bool reuse[2], rebuild[2];
    for (int s = 0; s < 2; ++s) {
        const bool listed = f.use_worklist[s] && f.n_work[s] != 0;
        reuse[s] = listed && k.list_valid[s] && f.block_is_list[s] && !(f.flags & ZRP_NO_LIST_REUSE);
        rebuild[s] = listed && !reuse[s];
    }
    // (a kept shadow pass launches nothing: a list it would have rebuilt stays invalid until a drawn pass rebuilds it)
    p.shadow_list_reuse = reuse[0]; p.shadow_list_rebuild = rebuild[0]; p.camera_list_reuse = reuse[1]; p.camera_list_rebuild = rebuild[1];

    // The shadow MAP is kept one level up: while the shadow pass's block, the casters (caster_epoch) and the map's buffer stand still, the
    // map of the last drawn pass is the map this frame would draw, bit for bit, and the pass launches nothing.  Contexts whose map is never
    // kept (every frame draws it): the host reduces or gathers a partitioned or caller-owned map in place; ZR_FLAG_NO_LIST_REUSE asks to
    // recompute what standing inputs would let the library keep; ZR_FLAG_SHADOW_OCCLUSION forces a variant of the pass for A/B, whose
    // per-frame history statistics are what its callers read.
    const bool shadow_keepable = !f.map_external && f.tile_world <= 1u && f.shadow_world <= 1u && f.stile_world <= 1u &&
                                 !(f.flags & (ZRP_NO_LIST_REUSE | ZRP_SHADOW_OCCLUSION));
    p.shadow_keep = shadow_keepable && k.smap_valid && k.smap_epoch == f.caster_epoch && f.shadow_is_map;
    p.shadow = p.shadow_keep ? ZR_LANE_NONE : ZR_LANE_HOST;
    // Shadow occlusion culling (k_shadow_occlusion): the first launch draws what was not hidden last frame, the rest is tested against the
    // map.  It pays when casters pile up behind each other: the test + the late launch cost what a quarter of config 3's rasteriser does
    // (0.1 meshlet-instances per texel: 25 % hidden, frame 2.7 % slower); the same spheres at 0.21 / 0.31 / 0.52 per texel: frame 2 /
    // 8 / 10.5 % faster (tools/occlusion_threshold.py); 1 M instances (10 per texel): 10 % - on by itself from one per five texels.
    p.shadow_occlusion = !p.shadow_keep && !(f.flags & ZRP_NO_SHADOW_OCCLUSION) && f.n_work[0] != 0 && f.SD >= 4u &&
                         ((f.flags & ZRP_SHADOW_OCCLUSION) || 5ull * f.n_work[0] >= (uint64_t)f.SD * f.SD);

    // Round 2 of the camera pass is kept the same way.  Round 1 draws the meshlet-instances that owned a pixel of the previous frame's
    // final key buffer; when this frame's camera-pass inputs are that frame's bit for bit (cam_same), whatever owned no pixel then owns
    // none now: the key buffer behind round 1 is already the frame's, and the frame enqueues no Hi-Z build, no k_select and no second
    // round.  Only when the frame before was settled (ZrFrameCarry::r2_settled) are round 2's statistics and per-tile counts, which a
    // keeping frame reports and plans with, those a drawn round 2 would give now: the frame after a camera cut draws round 2 from a stale
    // history (tens of millions of records at config 4 where the settled frame has a few); the frame after it draws both rounds once
    // more, and the rest of the rest keeps.  Never with ZR_FLAG_NO_LIST_REUSE, as above.  A rank of a tile-partitioned frame keeps it
    // like any other context: the statement is per pixel, and a rank's key buffer holds its own tiles only.
    p.cam_same = k.cam_prev_valid && k.cam_prev_epoch == f.camera_epoch && f.camera_is_prev;
    const bool round2_keep = !(f.flags & ZRP_NO_LIST_REUSE) && p.cam_same && k.r2_settled;
    // Two-pass occlusion culling: round 1 draws what owned a pixel last frame, a Hi-Z pyramid of the result rejects what it hides, round 2
    // draws the rest.  Without a history (first frame of a scene) or with ZR_FLAG_NO_HIZ everything is drawn at once.
    p.hiz_on = !(f.flags & ZRP_NO_HIZ) && f.n_work[1] != 0;
    const bool two = p.hiz_on && k.vis_history;
    // The record buckets are planned from the previous frame.  count_first: there is no usable plan (first frame of a scene, or the last
    // plan was made by a two-round frame and this round draws everything) - k_geom runs once more ahead of the round, counting only.
    p.count_first = !k.plan_valid || (!two && k.plan_two_round);
    p.rounds = !two ? ZR_ROUNDS_ONE : round2_keep && !p.count_first ? ZR_ROUNDS_TWO_KEPT : ZR_ROUNDS_TWO;

    // The camera pass is kept WHOLE, its GBuffer with it, one level further.  The lighting pass reads only the GBuffer planes and the
    // frame's XkView; the planes depend on the camera pass's inputs and on what the resolve reads beyond them (surface_epoch: texture
    // updates, the winner planes coming or going; materials, draw records and the skydome change through the scene, which bumps
    // camera_epoch).  After two drawn frames of one run of equal inputs both copies were resolved from these very inputs and are equal
    // bit for bit: the frame lights its parity's copy and launches nothing of the camera pipeline - no cull, round, k_mark, k_plan or
    // resolve, no statistics reset, nothing on the camera lane.  Not with a skydome or while a copy still waits for its overlay wipe
    // (the sky key plane is single-buffered).
    p.g_gen = k.g_gen + ((!p.cam_same || k.surf_prev_epoch != f.surface_epoch) ? 1u : 0u);
    const bool settled = round2_keep && !rebuild[1] && k.vis_history && k.plan_valid && f.n_work[1] != 0 && !(f.flags & ZRP_NO_HIZ);
    const bool copies = f.copy_gen[0] == p.g_gen && f.copy_gen[1] == p.g_gen && !f.copy_overlay[0] && !f.copy_overlay[1];
    p.camera_keep = settled && copies && !f.sky;
    p.camera = p.camera_keep ? ZR_LANE_NONE : lanes ? ZR_LANE_CAM : ZR_LANE_HOST;
    p.reset_stats = !p.camera_keep; p.reset_camera_list = !p.camera_keep && rebuild[1];

    // Where the resolve runs.  Nothing later on the camera lane of the same frame needs its planes: only the same frame's lighting pass
    // reads them, on the host's stream.  In a frame that keeps its shadow map that stream has nothing else to do, and the camera lane's
    // chain of launches is the frame's period: the resolve then goes to the host's stream, ahead of the lighting pass, and k_mark leaves
    // the next frame's camera lane the visibility history.  Only zr_render does this (a host may read the GBuffer after
    // zr_render_geometry, and the staged entry points run on one stream anyway), only on two lanes, and not with a skydome (its key plane
    // is single-buffered).  (shadow_keep already implies an unpartitioned context.)
    p.resolve_deferred = !p.camera_keep && lanes && render && p.shadow_keep && !f.sky;
    p.resolve = p.camera_keep ? ZR_LANE_NONE : p.resolve_deferred ? ZR_LANE_HOST : p.camera;

    // The lighting pass keeps, per pixel, what the moving point lights do not feed: ShadowFactor, Direct over the directional lights, RefC.
    // Their inputs are the pixel's GBuffer values, the shadow map, and a few hundred bytes of uniforms plus the cubemap.  A frame that keeps
    // its camera pass lights a GBuffer copy that is, bit for bit, every other copy of the same run (g_gen); a frame that keeps its map
    // lights from the map of one drawing frame (smap_frame; never a caller-owned or partitioned map: those are drawn every frame).  When
    // the plane was filled from that run, that map, these uniforms and this cubemap, the pass reads it; when the frame rests but the plane
    // does not match, the pass fills it - a resting frame by definition, so the moving-camera and moving-light loops never pay the stores.
    // The plane holds what a fill wrote: with the empty-pixel shortcut on, not the pixels that took it, and those are the same pixels on
    // every frame of the run - but a frame whose shortcut is off reads every pixel, and needs a fill that wrote them all.  All lighting
    // passes of a context run in order on the host's stream (p.lighting), so one plane serves the frames in flight.  Deferred shading
    // only; never with ZR_FLAG_NO_LIST_REUSE, as above.
    const bool light_rest = f.light_plane_ok && !(f.flags & ZRP_NO_LIST_REUSE) && f.shading != ZRP_SHADING_FORWARD && p.camera_keep && p.shadow_keep;
    const bool light_match = k.light_valid && k.light_g_gen == p.g_gen && k.light_smap_frame == k.smap_frame && f.light_uniforms_same &&
                             k.light_cube_gen == f.cube_gen && (k.light_all_px || f.light_empty_px);
    p.light_keep = light_rest && light_match; p.light_fill = light_rest && !light_match;
    p.light_args = p.light_keep && f.light_by_arg;

    // The head of a frame that keeps its camera pass has nothing to reset and runs where the frame is lit - or, where zr_render keeps the
    // map too (ZR_KEPT_HEAD_ON_LANE), on the idle lane, one-pixel launch included.  That launch reads the map, and the lane has waited for
    // the end of frame_no - 2 only: the map must have been drawn by that frame or an earlier one (a map drawn by the frame before, on the
    // host's stream, is behind nothing the lane has waited for).
    // A frame that is one launch (light_args) has no head at all: nothing to upload, nothing to launch ahead of the pass.  A frame that
    // fills the plane of a context with a slot (light_slot) fills the slot from its one-pixel launch, and the lighting pass of the frame
    // before may still be reading it: its head stays on the host's stream, behind that pass (one frame per rest).  A context without a
    // slot fills as it always did, head on the lane.
    const bool head_on_lane = kZrKeptHeadOnLane && p.camera_keep && render && p.shadow_keep && lanes && k.smap_frame + 2 <= f.frame_no &&
                              !p.light_args && !(p.light_fill && f.light_slot);
    p.head = p.camera_keep ? (head_on_lane ? ZR_LANE_CAM : ZR_LANE_HOST) : p.camera;
    // (the forward variant has no one-pixel launch: an empty pixel is the clear colour)
    p.one_pixel = f.shading == ZRP_SHADING_FORWARD || p.light_args ? ZR_LANE_NONE : head_on_lane ? ZR_LANE_CAM : ZR_LANE_HOST;

    // Waits at the head.  On the lane: this frame's copies of the double-buffered resources were last used two frames ago, on the host's
    // stream (read by the lighting pass, and before it the keys reset and the GBuffer written by the resolve where that ran there).
    // Consecutive camera pipelines share the triangle records, the plan and the lane's statistics and are ordered by running on ONE
    // stream: a frame on the lane that follows a camera pipeline on the host's stream waits for that frame's end.  The other way round the
    // host's stream has waited for ev_cam before that frame's lighting pass: the whole lane, k_plan included - unless ev_cam sat ahead of
    // k_plan (plan_behind_cam); then a camera pipeline on the host's stream waits for the lane's end here.  A frame that keeps its camera
    // pass touches nothing of the lane's or of its GBuffer copy: that wait, and the census's, are left to the next drawn frame.
    p.wait_end2 = p.head == ZR_LANE_CAM && f.frame_no >= 2;
    p.wait_end1 = p.head == ZR_LANE_CAM && f.frame_no >= 1 && k.gbuf_lane == ZR_LANE_HOST;
    p.wait_lane_end = !p.camera_keep && k.plan_behind_cam && p.head == ZR_LANE_HOST && f.has_lane;
    p.ids_taken = !p.camera_keep && f.copy_ids_wait[f.frame_no & 1u];
    p.wait_ids = p.ids_taken && p.head == ZR_LANE_CAM;      // (the census runs on the host's stream)

    // Every event record / wait is a barrier packet, worth 5-10 us of bubble on the stream it sits on, and the host's stream (lighting ->
    // shadow pipeline -> lighting ...) is the lane the frame rate hangs on: it waits for the camera lane once per frame, before the
    // lighting pass, and for nothing else.
    p.ev_cam = p.resolve_deferred ? ZR_EVCAM_BEHIND_MARK
             : kZrEvCamAheadOfPlan && render && p.camera == ZR_LANE_CAM ? ZR_EVCAM_BEHIND_RESOLVE
             : head_on_lane ? ZR_EVCAM_BEHIND_ONE_PIXEL
             : p.camera == ZR_LANE_CAM ? ZR_EVCAM_LANE_END : ZR_EVCAM_NONE;
    p.host_waits_ev_cam = p.ev_cam != ZR_EVCAM_NONE;      // (wherever it is recorded, it is recorded on the lane)
    // ev_join (zr_stream_wait_shadow: a host that puts a collective behind the shadow pass): not in zr_render's own two-lane frames
    p.ev_join = !(lanes && render);

    return p;
}

// The carry after `stage` of plan p has been enqueued completely.  HEAD (called once the frame is planned, ahead of its first launch)
// also takes back what the frame is about to overwrite - a list it rebuilds, a map or a camera pass it draws: a stage that fails part-way
// leaves them invalid, and nothing is ever kept that was not completely enqueued.
static inline ZrFrameCarry zr_frame_carry(const ZrFrameCarry& before, const ZrFrameFacts& f, const ZrFramePlan& p, ZrStage stage)
{
    ZrFrameCarry k = before;
    switch (stage) {
    case ZR_STAGE_HEAD:
        k.g_gen = p.g_gen; k.surf_prev_epoch = f.surface_epoch;
        if (p.shadow_list_rebuild) k.list_valid[0] = false;
        if (p.camera_list_rebuild) k.list_valid[1] = false;
        if (!p.shadow_keep) k.smap_valid = false;
        if (!p.camera_keep) { k.r2_settled = k.cam_prev_valid = false; k.plan_behind_cam = false; }      // (the head has waited for the lane's end where it had to)
        if (p.light_fill) k.light_valid = false;
        break;
    case ZR_STAGE_SHADOW:          // a drawn pass: the map is this frame's
        if (p.shadow_list_rebuild) k.list_valid[0] = true;
        if (p.shadow_occlusion) k.sflag_history = true;
        k.smap_epoch = f.caster_epoch; k.smap_frame = f.frame_no; k.smap_valid = true;
        break;
    case ZR_STAGE_CAMERA:          // a drawn pass, up to its k_plan
        if (p.camera_list_rebuild) k.list_valid[1] = true;
        k.gbuf_lane = p.camera;
        k.plan_behind_cam = p.ev_cam == ZR_EVCAM_BEHIND_MARK || p.ev_cam == ZR_EVCAM_BEHIND_RESOLVE;
        if (f.n_work[1] != 0) { k.plan_valid = true; k.plan_two_round = p.rounds != ZR_ROUNDS_ONE; }      // (k_plan ran: the next frame's buckets)
        k.r2_settled = p.rounds != ZR_ROUNDS_ONE && p.cam_same;
        k.cam_prev_epoch = f.camera_epoch; k.cam_prev_valid = k.vis_history = p.hiz_on;
        break;
    case ZR_STAGE_LIGHTING:        // a pass that filled the plane: it is this frame's
        if (p.light_fill) {
            k.light_valid = true; k.light_all_px = !f.light_empty_px;
            k.light_g_gen = p.g_gen; k.light_smap_frame = k.smap_frame; k.light_cube_gen = f.cube_gen;
        }
        break;
    }
    return k;
}
