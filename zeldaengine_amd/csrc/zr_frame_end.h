// zr_frame_end.h — the end-of-frame event, recorded where someone will ask for it ("The schedule").  Every lighting
// pass runs on the host's stream in frame order, and every stream wait for a frame's end is made on another stream: an event recorded
// LATER on the host's stream is a valid, merely conservative, stand-in for any earlier frame's end.  So a frame in a run of one-launch
// frames records its end only every `every`-th frame (ZR_REST_END_EVERY; 1: every frame does), and a reader that asks for an end nobody
// recorded gets the stream's tail, recorded then.  This header is the rule and its state: which frame each slot of the ring was last
// recorded for, which end a reader is handed, which end a one-launch frame paces the host on, which run of frames a period is the mean
// of.  Plain C++17 and nothing of HIP, like zr_settle.h: tests/frame_end_check.cpp compiles this header alone and sweeps it without a GPU.
#pragma once

#include <cstdint>

constexpr int kZrEndRing = 512;          // zr_ctx::END_RING: the ring of end-of-frame events
constexpr int kZrViewRing = 4;           // zr_ctx::VIEW_RING: how far the uniform ring lets the host run ahead of the device
constexpr uint32_t kZrEndEveryMax = 64;  // ZR_REST_END_EVERY is clamped to 1 .. this (the ring holds many such runs)
// `every` where ZR_REST_END_EVERY is not set (measured: DESIGN.md section 7, "Only the events someone reads")
#ifndef ZR_REST_END_EVERY_DEFAULT
#define ZR_REST_END_EVERY_DEFAULT 8u
#endif

// slot[i]: frame + 1 of the frame the slot's event was last recorded for (0: none yet) - a slot is read only where that is the frame
// asked for.  newest: frame + 1 of the newest recorded end.  synced: frame + 1 of the newest end a one-launch frame synchronised the host
// on.  prev_args: the frame enqueued last was planned as one launch (ZrFramePlan::light_args).
struct ZrEndState {
    uint64_t slot[kZrEndRing] = {};
    uint64_t newest = 0, synced = 0;
    uint32_t every = 1;
    bool prev_args = false;
};

static inline bool zr_end_recorded(const ZrEndState& s, uint64_t f) { return s.slot[f % kZrEndRing] == f + 1; }

// Whether frame f's lighting pass records its end: always, unless the frame is one launch, its predecessor was too, and f is no
// multiple of `every`.  (Moving loops never rest: they record every frame.)
static inline bool zr_end_records(const ZrEndState& s, uint64_t f, bool light_args) { return !(light_args && s.prev_args && f % s.every != 0); }

// Frame f's lighting pass is enqueued; `recorded`: its end with it, into slot f % kZrEndRing.
static inline void zr_end_enqueued(ZrEndState* s, uint64_t f, bool light_args, bool recorded)
{
    if (recorded) { s->slot[f % kZrEndRing] = f + 1; s->newest = f + 1; }
    s->prev_args = light_args;
}

// "The end of frame f", asked for when frames 0 .. frame_no - 1 are enqueued (f < frame_no): the event of slot `frame % kZrEndRing`,
// which holds the end of `frame` >= f.  record: nothing at or behind f is recorded - the caller records the host's stream's tail into
// that slot first, the newest frame's, which covers every frame up to it (the state already says so).
struct ZrEndAsk { uint64_t frame = 0; bool record = false; };
static inline ZrEndAsk zr_end_ask(ZrEndState* s, uint64_t f, uint64_t frame_no)
{
    ZrEndAsk a;
    if (zr_end_recorded(*s, f)) { a.frame = f; return a; }
    if (s->newest > f + 1) { a.frame = s->newest - 1; return a; }      // (a later end: its slot is still its own - nothing newer was recorded)
    a.frame = frame_no - 1; a.record = true;
    s->slot[a.frame % kZrEndRing] = a.frame + 1; s->newest = a.frame + 1;
    return a;
}

// Pacing of a one-launch frame (it uploads nothing, so the uniform ring does not pace it): the frame whose end the host synchronises on
// before it enqueues frame_no, as frame + 1 - the newest recorded end at or before frame_no - kZrViewRing - or 0: none yet, or already
// synchronised on.  The host is then never more than kZrViewRing + every - 1 frames ahead of the device.
static inline uint64_t zr_end_pace(ZrEndState* s, uint64_t frame_no)
{
    if (frame_no < (uint64_t)kZrViewRing) return 0;
    uint64_t g = frame_no - kZrViewRing;
    for (uint32_t n = 0; n < s->every; ++n, --g) {
        if (zr_end_recorded(*s, g)) {
            if (g + 1 <= s->synced) return 0;
            s->synced = g + 1;
            return g + 1;
        }
        if (g == 0) break;
    }
    return 0;
}

// The run frame f's period is the mean of: (a, b], a < f <= b the recorded ends nearest to f on either side - the period is the time from
// a's event to b's over b - a frames, and the sum over any window whose ends are recorded is exact.  False: one of the two is no longer
// (or not yet) in the ring.
static inline bool zr_end_run(const ZrEndState& s, uint64_t f, uint64_t* a, uint64_t* b)
{
    if (f == 0 || f + 1 > s.newest) return false;
    uint64_t hi = f, lo = f - 1;
    while (!zr_end_recorded(s, hi)) { if (hi + 1 >= s.newest) return false; ++hi; }
    for (int n = 0; !zr_end_recorded(s, lo); ++n, --lo) if (lo == 0 || n >= kZrEndRing) return false;
    if (hi - lo >= (uint64_t)kZrEndRing) return false;      // (lo's slot would be hi's)
    *a = lo; *b = hi;
    return true;
}
