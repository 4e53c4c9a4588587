// zr_timed.h — which pass events a timed frame records, and what each ZR_PASS_* figure is read from ("The
// schedule").  A record is a barrier packet on the stream it sits on, so a stage the plan does not run records nothing: its figures read
// exactly 0, and the read-out never meets an event its sample did not record (a ring slot's other events are 64 samples old, or were never
// recorded at all).  zr_timed_rule() is the whole rule, from the frame's plan alone: frame_begin stores its result with the sample,
// TIMED() records what the set holds, zr_get_pass_times_avg and zr_get_frame_latencies read what the figures name.  Plain C++17 and
// nothing of HIP, like zr_settle.h: tests/timed_plan_check.cpp compiles this header alone and sweeps it without a GPU.
#pragma once

#include "zr_frame_plan.h"

// One timed frame's events, in the order of the frame graph: frame_begin; the shadow pipeline's bins filled, its map drawn; the camera
// pipeline's start, its cull, round 1, Hi-Z build + k_select, round 2 + skydome; the end of k_mark (camera lane) and the start of the
// resolve where that runs on the host's stream; the resolve's end, the lighting's.
enum TimedEvent { EV_BEGIN, EV_SHADOW_BINS, EV_SHADOW, EV_CULL, EV_ROUND1, EV_HIZ, EV_ROUND2, EV_RESOLVE, EV_LIGHTING, EV_CAMERA,
                  EV_MARK, EV_HOST_RESOLVE, EV_COUNT };

// The figures, under names of this header's own (zelda_render.h has the ZR_PASS_* originals; zr_readback.cpp asserts that they agree).
enum ZrTimedFigure { ZRT_CULL_SHADOW, ZRT_SHADOW, ZRT_CULL_CAMERA, ZRT_GBUFFER, ZRT_HIZ, ZRT_GBUFFER2, ZRT_RESOLVE, ZRT_LIGHTING, ZRT_COMPOSITE,
                     ZRT_TOTAL, ZRT_COUNT };

// A figure is the sum of n spans, each the time from one recorded event to another; n = 0: the figure reads 0.
struct ZrTimedSpan { uint8_t from = 0, to = 0; };
struct ZrTimedReading { uint8_t n = 0; ZrTimedSpan span[2]; };
// recorded: bit e set = the frame records event e, on the stream of lane[e] (never ZR_LANE_NONE for a recorded event).
struct ZrTimedRule {
    uint32_t recorded = 0;
    ZrLane lane[EV_COUNT] = {};
    ZrTimedReading fig[ZRT_COUNT];
    bool records(int e) const { return (recorded >> e & 1u) != 0; }
};

static inline ZrTimedRule zr_timed_rule(const ZrFramePlan& p)
{
    ZrTimedRule r;
    const auto record = [&r](TimedEvent e, ZrLane on) { r.recorded |= 1u << e; r.lane[e] = on; };
    const auto reads = [&r](ZrTimedFigure g, TimedEvent from, TimedEvent to) {
        ZrTimedSpan& s = r.fig[g].span[r.fig[g].n++];
        s.from = (uint8_t)from; s.to = (uint8_t)to;
    };
    const bool camera = p.camera != ZR_LANE_NONE, shadow = p.shadow != ZR_LANE_NONE;

    // Every frame: its begin, where its head runs, and the end of its lighting pass.
    record(EV_BEGIN, p.head); record(EV_LIGHTING, p.lighting);
    reads(ZRT_TOTAL, EV_BEGIN, EV_LIGHTING);

    // The shadow pipeline runs on the host's stream.  A kept map ran none: both figures read 0.  A frame that draws its camera pass records
    // the set it always did - the two marks of a kept map too, back to back on the host's stream, read by nobody; a frame that keeps camera
    // pass and map records neither.
    if (shadow || camera) { record(EV_SHADOW_BINS, ZR_LANE_HOST); record(EV_SHADOW, ZR_LANE_HOST); }
    if (shadow) { reads(ZRT_CULL_SHADOW, EV_BEGIN, EV_SHADOW_BINS); reads(ZRT_SHADOW, EV_SHADOW_BINS, EV_SHADOW); }

    if (camera) {
        // The camera pipeline, on its lane.  (A frame that draws one round or keeps round 2 records EV_HIZ and EV_ROUND2 all the same, back
        // to back; round 2 kept: its two figures read 0.)
        record(EV_CAMERA, p.camera); record(EV_CULL, p.camera); record(EV_ROUND1, p.camera); record(EV_HIZ, p.camera); record(EV_ROUND2, p.camera);
        reads(ZRT_CULL_CAMERA, EV_CAMERA, EV_CULL); reads(ZRT_GBUFFER, EV_CULL, EV_ROUND1);
        if (p.rounds != ZR_ROUNDS_TWO_KEPT) { reads(ZRT_HIZ, EV_ROUND1, EV_HIZ); reads(ZRT_GBUFFER2, EV_HIZ, EV_ROUND2); }
        if (p.resolve_deferred) {
            // the resolve on the host's stream: k_mark on the camera lane + the resolve itself, each between two records on the stream it
            // ran on (never across the wait between the lanes)
            record(EV_MARK, p.camera); record(EV_HOST_RESOLVE, p.resolve); record(EV_RESOLVE, p.resolve);
            reads(ZRT_RESOLVE, EV_ROUND2, EV_MARK); reads(ZRT_RESOLVE, EV_HOST_RESOLVE, EV_RESOLVE);
        } else {
            record(EV_RESOLVE, p.resolve);
            reads(ZRT_RESOLVE, EV_ROUND2, EV_RESOLVE);
        }
        reads(ZRT_LIGHTING, EV_RESOLVE, EV_LIGHTING);      // (the resolve's end is the lighting's start mark)
    } else if (p.light_args) {
        // One launch: nothing is enqueued between EV_BEGIN and it, and both are on the host's stream - the begin is the start mark.  (Where
        // lighting_pass demotes such a frame, a diagnostic path, its late uniform upload falls into this span.)
        reads(ZRT_LIGHTING, EV_BEGIN, EV_LIGHTING);
    } else {
        // The camera pass kept whole: nothing of it ran, and one mark where it would have stood, on the stream that lights the frame, starts
        // the lighting's span - ahead of the wait for the lane and the one-pixel launch, as ever.
        record(EV_RESOLVE, p.lighting);
        reads(ZRT_LIGHTING, EV_RESOLVE, EV_LIGHTING);
    }
#ifdef ZR_TIMED_DIAG      // diagnosis only: the kept frames of one kind record what they recorded before the rule
    if (!camera && ((ZR_TIMED_DIAG & 1) ? p.light_args : !p.light_args)) {
        const TimedEvent old[] = { EV_SHADOW_BINS, EV_SHADOW, EV_CAMERA, EV_CULL, EV_ROUND1, EV_HIZ, EV_ROUND2, EV_RESOLVE };
        for (TimedEvent e : old) if (!r.records(e)) record(e, ZR_LANE_HOST);
    }
#endif
    return r;
}
