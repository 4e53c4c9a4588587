// timed_plan_check.cpp — which pass events a timed frame records and what its figures read (csrc/zr_timed.h), run without a GPU:
// tests/test_timed_plan.py compiles this file, runs it and holds what it prints against expectations written out there.
//
//   1. A scripted sequence of frames through zr_frame_plan / zr_frame_carry as the host drives them - two drawn frames, the fill, three
//      one-launch frames, a light move, a camera move: "== story", then per frame the plan's shape, the record count and the set.
//   2. The rule's invariants over every combination of the facts and carry bits that decide which stages a frame runs, where, and whether
//      it is one launch: "swept <combinations>", "seen ..." for the shapes met, "broken <n>"; exit status 1 and a line per broken invariant.
#include "zr_timed.h"

#include <cstdio>

static const char* const kEvName[EV_COUNT] = { "begin", "shadow_bins", "shadow", "cull", "round1", "hiz", "round2", "resolve", "lighting", "camera",
                                               "mark", "host_resolve" };
static const char* lane_name(ZrLane l) { return l == ZR_LANE_NONE ? "none" : l == ZR_LANE_HOST ? "host" : "cam"; }
static int count(uint32_t set) { int n = 0; for (; set; set &= set - 1u) ++n; return n; }
static uint32_t bit(int e) { return 1u << e; }

// ---------------------------------------------------------------------------------------------- the story

struct Host {
    ZrFrameFacts f; ZrFrameCarry k;
    int shadow_block = 1, camera_block = 1, smap_key = 0, cam_prev_key = 0;
    uint64_t frame_no = 0, copy_gen[2] = { 0, 0 };
};

static void frame(Host& h)
{
    ZrFrameFacts& f = h.f;
    f.frame_no = h.frame_no;
    f.shadow_is_map = h.smap_key == h.shadow_block; f.camera_is_prev = h.cam_prev_key == h.camera_block;
    f.block_is_list[0] = f.block_is_list[1] = true;
    for (int i = 0; i < 2; ++i) f.copy_gen[i] = h.copy_gen[i];
    const ZrFramePlan p = zr_frame_plan(f, h.k);
    h.k = zr_frame_carry(h.k, f, p, ZR_STAGE_HEAD);
    if (p.shadow != ZR_LANE_NONE) { h.smap_key = h.shadow_block; h.k = zr_frame_carry(h.k, f, p, ZR_STAGE_SHADOW); }
    if (p.camera != ZR_LANE_NONE) { h.copy_gen[h.frame_no & 1u] = p.g_gen; h.cam_prev_key = h.camera_block; h.k = zr_frame_carry(h.k, f, p, ZR_STAGE_CAMERA); }
    h.k = zr_frame_carry(h.k, f, p, ZR_STAGE_LIGHTING);
    const ZrTimedRule r = zr_timed_rule(p);
    printf("frame=%llu shadow=%s camera=%s args=%d fill=%d n=%d set=", (unsigned long long)h.frame_no, lane_name(p.shadow), lane_name(p.camera),
           (int)p.light_args, (int)p.light_fill, count(r.recorded));
    for (int e = 0, first = 1; e < EV_COUNT; ++e) if (r.records(e)) { printf("%s%s", first ? "" : ",", kEvName[e]); first = 0; }
    printf(" lighting_from=%s\n", kEvName[r.fig[ZRT_LIGHTING].span[0].from]);
    h.frame_no++;
}

static void story()
{
    puts("== story");
    Host h;
    h.f.SD = 256; h.f.n_work[0] = h.f.n_work[1] = 1000; h.f.entry = ZR_ENTRY_RENDER; h.f.has_lane = true;
    h.f.light_plane_ok = h.f.light_uniforms_same = h.f.light_by_arg = h.f.light_slot = true;
    for (int i = 0; i < 6; ++i) frame(h);      // drawn, drawn, the fill, three frames of one launch
    h.shadow_block = 2; frame(h);              // the light moved: the map drawn, the camera pass kept
    h.camera_block = 2; frame(h);              // the camera moved
}

// ---------------------------------------------------------------------------------------------- the sweep

enum Dim { D_NO_HIZ, D_SERIAL, D_NO_LIST_REUSE, D_SKY, D_FORWARD, D_HAS_LANE, D_SHADOW_IS_MAP, D_CAMERA_IS_PREV, D_N_WORK_CAMERA, D_SMAP_VALID, D_SMAP_AGE,
           D_R2_SETTLED, D_PLAN_VALID, D_VIS_HISTORY, D_PLANE_OK, D_LIGHT_VALID, D_BY_ARG, D_SLOT, D_FRAME_NO, D_COPY_GEN, D_ENTRY, D_COUNT };
static const int kValues[D_COUNT] = { 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2,  2, 2, 2, 2, 2, 2, 2, 2, 2, 3 };

struct Case { ZrFrameFacts f; ZrFrameCarry k; };

// The one-launch resting zr_render frame: everything stands, everything is kept, the plane is filled and matches.
static Case resting()
{
    Case c;
    c.f.SD = 256; c.f.n_work[0] = c.f.n_work[1] = 1000; c.f.entry = ZR_ENTRY_RENDER; c.f.has_lane = true; c.f.frame_no = 5;
    c.f.caster_epoch = c.f.camera_epoch = c.f.surface_epoch = 7;
    c.f.shadow_is_map = c.f.camera_is_prev = c.f.block_is_list[0] = c.f.block_is_list[1] = true;
    c.f.copy_gen[0] = c.f.copy_gen[1] = 5;
    c.f.light_plane_ok = c.f.light_uniforms_same = c.f.light_by_arg = c.f.light_slot = true;
    c.k.smap_valid = c.k.cam_prev_valid = c.k.r2_settled = c.k.plan_valid = c.k.plan_two_round = c.k.vis_history = c.k.sflag_history = true;
    c.k.list_valid[0] = c.k.list_valid[1] = true;
    c.k.smap_epoch = c.k.cam_prev_epoch = c.k.surf_prev_epoch = 7; c.k.smap_frame = 0; c.k.g_gen = 5; c.k.gbuf_lane = ZR_LANE_CAM;
    c.k.light_valid = true; c.k.light_g_gen = 5; c.k.light_smap_frame = 0;
    return c;
}

static void flag(Case& c, uint32_t b, int v) { c.f.flags = v ? c.f.flags | b : c.f.flags & ~b; }
// (D_FRAME_NO comes before D_SMAP_AGE takes effect: set() is applied in the order of the enum's values below)
static void set(Case& c, Dim d, int v)
{
    switch (d) {
    case D_NO_HIZ: flag(c, ZRP_NO_HIZ, v); break;
    case D_SERIAL: flag(c, ZRP_SERIAL_PASSES, v); break;
    case D_NO_LIST_REUSE: flag(c, ZRP_NO_LIST_REUSE, v); break;
    case D_SKY: c.f.sky = v != 0; break;
    case D_FORWARD: c.f.shading = v ? ZRP_SHADING_FORWARD : 0u; break;
    case D_HAS_LANE: c.f.has_lane = v == 0; break;
    case D_SHADOW_IS_MAP: c.f.shadow_is_map = v == 0; break;
    case D_CAMERA_IS_PREV: c.f.camera_is_prev = v == 0; break;
    case D_N_WORK_CAMERA: c.f.n_work[1] = v ? 0u : 1000u; break;
    case D_SMAP_VALID: c.k.smap_valid = v == 0; break;
    case D_SMAP_AGE: c.k.smap_frame = c.k.light_smap_frame = v ? c.f.frame_no - 1 : c.f.frame_no - 2; break;      // (the map drawn by the frame before: no head on the lane)
    case D_R2_SETTLED: c.k.r2_settled = v == 0; break;
    case D_PLAN_VALID: c.k.plan_valid = v == 0; break;
    case D_VIS_HISTORY: c.k.vis_history = v == 0; break;
    case D_PLANE_OK: c.f.light_plane_ok = v == 0; break;
    case D_LIGHT_VALID: c.k.light_valid = v == 0; break;
    case D_BY_ARG: c.f.light_by_arg = v == 0; break;
    case D_SLOT: c.f.light_slot = v == 0; break;
    case D_FRAME_NO: c.f.frame_no = v ? 2u : 5u; break;
    case D_COPY_GEN: c.f.copy_gen[1] = v ? 4 : 5; break;      // (1: a copy of an earlier run - the camera pass is drawn once more)
    case D_ENTRY: c.f.entry = (ZrEntry)v; break;
    default: break;
    }
}

static int g_broken = 0;
static unsigned long long g_seen[6] = { 0, 0, 0, 0, 0, 0 };      // one launch / kept-kept not by argument / kept camera, drawn map / drawn camera / resolve deferred / round 2 kept in a drawn pass

#define HOLDS(cond) do { if (!(cond)) { if (g_broken++ < 20) printf("broken: %s (line %d) flags=%u entry=%d frame=%llu\n", #cond, __LINE__, f.flags, (int)f.entry, (unsigned long long)f.frame_no); } } while (0)
#define IMPLIES(a, b) HOLDS(!(a) || (b))

// What the frame records where it draws its camera pass, written out from the host as it stood before the rule (frame_begin, shadow_pass /
// shadow_draw, gbuffer_pass, deferred_resolve, lighting_pass): every event but the three of a resolve on the host's stream, and those too
// where the resolve runs there.
static uint32_t drawn_camera_set(const ZrFramePlan& p)
{
    uint32_t s = bit(EV_BEGIN) | bit(EV_SHADOW_BINS) | bit(EV_SHADOW) | bit(EV_CAMERA) | bit(EV_CULL) | bit(EV_ROUND1) | bit(EV_HIZ) | bit(EV_ROUND2) |
                 bit(EV_RESOLVE) | bit(EV_LIGHTING);
    if (p.resolve_deferred) s |= bit(EV_MARK) | bit(EV_HOST_RESOLVE);
    return s;
}
// ... and the stream each of them sat on, as the passes chose it
static ZrLane drawn_camera_lane(const ZrFramePlan& p, int e)
{
    switch (e) {
    case EV_BEGIN: return p.head;
    case EV_SHADOW_BINS: case EV_SHADOW: return ZR_LANE_HOST;      // (lane_stream(p.shadow) of a drawn map, c->stream of a kept one)
    case EV_HOST_RESOLVE: return p.resolve;
    case EV_RESOLVE: return p.resolve_deferred ? p.resolve : p.camera;
    case EV_LIGHTING: return p.lighting;
    default: return p.camera;
    }
}

static void check(const Case& c)
{
    const ZrFrameFacts& f = c.f;
    const ZrFramePlan p = zr_frame_plan(f, c.k);
    const ZrTimedRule r = zr_timed_rule(p);
    const bool camera = p.camera != ZR_LANE_NONE, shadow = p.shadow != ZR_LANE_NONE;
    g_seen[0] += p.light_args; g_seen[1] += !camera && !shadow && !p.light_args; g_seen[2] += !camera && shadow; g_seen[3] += camera;
    g_seen[4] += p.resolve_deferred; g_seen[5] += camera && p.rounds == ZR_ROUNDS_TWO_KEPT;

    // every event a figure reads is in the recorded set, on a stream; nothing outside the set has one
    for (int g = 0; g < ZRT_COUNT; ++g) {
        HOLDS(r.fig[g].n <= 2);
        for (int i = 0; i < r.fig[g].n; ++i) HOLDS(r.records(r.fig[g].span[i].from) && r.records(r.fig[g].span[i].to));
    }
    for (int e = 0; e < EV_COUNT; ++e) HOLDS(r.records(e) == (r.lane[e] != ZR_LANE_NONE));
    HOLDS(r.recorded >> EV_COUNT == 0u);
    // a figure reads 0 exactly where its stage did not run (round 2 and Hi-Z: also where a drawn pass keeps round 2)
    HOLDS((r.fig[ZRT_CULL_SHADOW].n == 0) == !shadow && (r.fig[ZRT_SHADOW].n == 0) == !shadow);
    HOLDS((r.fig[ZRT_CULL_CAMERA].n == 0) == !camera && (r.fig[ZRT_GBUFFER].n == 0) == !camera && (r.fig[ZRT_RESOLVE].n == 0) == !camera);
    HOLDS((r.fig[ZRT_HIZ].n == 0) == (!camera || p.rounds == ZR_ROUNDS_TWO_KEPT) && (r.fig[ZRT_GBUFFER2].n == 0) == (!camera || p.rounds == ZR_ROUNDS_TWO_KEPT));
    HOLDS(r.fig[ZRT_LIGHTING].n == 1 && r.fig[ZRT_TOTAL].n == 1 && r.fig[ZRT_COMPOSITE].n == 0);
    // the frame's span and the lighting's end where they always did
    HOLDS(r.records(EV_BEGIN) && r.records(EV_LIGHTING) && r.lane[EV_BEGIN] == p.head && r.lane[EV_LIGHTING] == p.lighting);
    HOLDS(r.fig[ZRT_TOTAL].span[0].from == EV_BEGIN && r.fig[ZRT_TOTAL].span[0].to == EV_LIGHTING && r.fig[ZRT_LIGHTING].span[0].to == EV_LIGHTING);
    // Both events of a span on one stream.  Three spans cross streams, as they did before the rule: frame_begin -> the bins (the head on the
    // camera lane, the shadow pipeline on the host's stream), the lane's resolve -> the lighting's end (a drawn camera pass on the lane), and
    // the frame's whole span where its head runs on the lane.
    for (int g = 0; g < ZRT_COUNT; ++g)
        for (int i = 0; i < r.fig[g].n; ++i) {
            const int a = r.fig[g].span[i].from, b = r.fig[g].span[i].to;
            const bool may_cross = (g == ZRT_CULL_SHADOW && p.head == ZR_LANE_CAM) || (g == ZRT_LIGHTING && camera && p.resolve == ZR_LANE_CAM) ||
                                   (g == ZRT_TOTAL && p.head == ZR_LANE_CAM);
            IMPLIES(!may_cross, r.lane[a] == r.lane[b]);
        }
    IMPLIES(p.light_args, r.lane[EV_BEGIN] == ZR_LANE_HOST && r.lane[EV_LIGHTING] == ZR_LANE_HOST);
    // a frame that draws its camera pass: the set and the streams it always had
    if (camera) {
        HOLDS(r.recorded == drawn_camera_set(p));
        for (int e = 0; e < EV_COUNT; ++e) IMPLIES(r.records(e), r.lane[e] == drawn_camera_lane(p, e));
        HOLDS(r.fig[ZRT_LIGHTING].span[0].from == EV_RESOLVE);
        HOLDS(r.fig[ZRT_RESOLVE].n == (p.resolve_deferred ? 2 : 1));
    }
    // the three kept shapes
    IMPLIES(p.light_args, r.recorded == (bit(EV_BEGIN) | bit(EV_LIGHTING)) && r.fig[ZRT_LIGHTING].span[0].from == EV_BEGIN);
    IMPLIES(!camera && !shadow && !p.light_args, r.recorded == (bit(EV_BEGIN) | bit(EV_RESOLVE) | bit(EV_LIGHTING)));
    IMPLIES(!camera && shadow, r.recorded == (bit(EV_BEGIN) | bit(EV_SHADOW_BINS) | bit(EV_SHADOW) | bit(EV_RESOLVE) | bit(EV_LIGHTING)));
    IMPLIES(!camera && !p.light_args, r.fig[ZRT_LIGHTING].span[0].from == EV_RESOLVE && r.lane[EV_RESOLVE] == p.lighting);
    IMPLIES(!camera, !r.records(EV_CAMERA) && !r.records(EV_CULL) && !r.records(EV_ROUND1) && !r.records(EV_HIZ) && !r.records(EV_ROUND2) &&
                     !r.records(EV_MARK) && !r.records(EV_HOST_RESOLVE));
    IMPLIES(!camera && !shadow, !r.records(EV_SHADOW_BINS) && !r.records(EV_SHADOW));
}

int main()
{
    story();
    int v[D_COUNT] = { 0 };
    unsigned long long visited = 0;
    for (;;) {
        Case c = resting();
        set(c, D_FRAME_NO, v[D_FRAME_NO]);
        for (int d = 0; d < D_COUNT; ++d) if (d != D_FRAME_NO) set(c, (Dim)d, v[d]);
        check(c);
        ++visited;
        int i = 0;
        while (i < D_COUNT && ++v[i] == kValues[i]) v[i++] = 0;
        if (i == D_COUNT) break;
    }
    printf("swept %llu\n", visited);
    printf("seen one_launch=%llu kept_kept=%llu kept_camera_drawn_map=%llu drawn_camera=%llu resolve_deferred=%llu round2_kept_drawn=%llu\n",
           g_seen[0], g_seen[1], g_seen[2], g_seen[3], g_seen[4], g_seen[5]);
    printf("broken %d\n", g_broken);
    return g_broken ? 1 : 0;
}
