// frame_end_check.cpp — the end-of-frame event recorded where someone will ask for it (csrc/zr_frame_end.h), run without a GPU:
// tests/test_frame_end.py compiles this file, runs it and holds what it prints against expectations written out there.
//
// A model of the host's stream beside the rule: every lighting pass and every event record gets its place in stream order, and the model
// keeps for itself which frame each slot's event was really recorded for.  Frames are of three kinds - one launch, another resting frame
// (no upload by argument: it waits for the end of the frame two before, like a drawn one), drawn - and between them a reader may ask for
// the end of the frame enqueued last or of the one before it (a texture update, a frame's head after a change of lanes).
//   "== story": twelve frames and two readers with every = 4, a line per step.
//   "swept every=<R> ...": every sequence of seven steps of the five kinds, begun at frame 0 and behind prefixes that put the ring's wrap
//   inside the sequence, and one pseudo-random sequence over several turns of the ring; "broken <n>", exit status 1 if an invariant fails.
#include "zr_frame_end.h"

#include <cstdio>
#include <vector>

enum Kind { ONE_LAUNCH, OTHER_REST, DRAWN, ASK_LAST, ASK_BEFORE, KINDS };
static const char* const kKind[KINDS] = { "one_launch", "other_rest", "drawn", "ask_last", "ask_before" };

static int g_broken = 0;
#define HOLDS(cond) do { if (!(cond)) { if (g_broken++ < 20) printf("broken: %s (line %d) every=%u frame_no=%llu\n", #cond, __LINE__, m.s.every, (unsigned long long)m.frame_no); } } while (0)

struct Model {
    ZrEndState s;
    uint64_t frame_no = 0, tail = 0;            // frames enqueued; places handed out on the host's stream
    std::vector<uint64_t> pass;                 // pass[f]: the place of frame f's lighting pass
    uint64_t ev_place[kZrEndRing] = {}, ev_frame[kZrEndRing] = {};      // the slot's event: where it was recorded, and for which frame + 1
    uint64_t host_synced = 0;                   // frame + 1 of the newest end the host waited for
    unsigned long long asks = 0, stand_ins = 0, recorded_now = 0, sparse = 0, paced = 0;
    bool print = false;
};

static void record(Model& m, uint64_t f) { m.ev_place[f % kZrEndRing] = ++m.tail; m.ev_frame[f % kZrEndRing] = f + 1; }

// a reader asks for the end of frame f
static void ask(Model& m, uint64_t f)
{
    const ZrEndAsk a = zr_end_ask(&m.s, f, m.frame_no);
    if (a.record) { HOLDS(a.frame == m.frame_no - 1); record(m, a.frame); m.recorded_now++; }
    m.asks++; m.stand_ins += a.frame != f;
    const int slot = (int)(a.frame % kZrEndRing);
    HOLDS(a.frame >= f && a.frame < m.frame_no);
    HOLDS(m.ev_frame[slot] == a.frame + 1);          // never a slot that holds another frame's event
    HOLDS(m.ev_place[slot] > m.pass[f]);             // recorded behind frame f's lighting pass, in stream order
    if (m.print) printf("frame_no=%llu kind=ask f=%llu handed=%llu recorded_now=%d\n", (unsigned long long)m.frame_no, (unsigned long long)f, (unsigned long long)a.frame, (int)a.record);
}

static void step(Model& m, Kind k)
{
    if (k == ASK_LAST || k == ASK_BEFORE) {
        const uint64_t back = k == ASK_LAST ? 1 : 2;
        if (m.frame_no >= back) ask(m, m.frame_no - back);
        return;
    }
    const uint64_t f = m.frame_no;
    const bool args = k == ONE_LAUNCH;
    if (args) {
        const uint64_t pace = zr_end_pace(&m.s, f);
        if (pace) { HOLDS(m.ev_frame[(pace - 1) % kZrEndRing] == pace && pace > m.host_synced && pace + kZrViewRing <= f + 1); m.host_synced = pace; m.paced++; }
        // the host is never more than VIEW_RING + every - 1 frames ahead of the newest end it has synchronised on
        if (f >= (uint64_t)kZrViewRing) HOLDS(m.host_synced != 0 && f - (m.host_synced - 1) <= (uint64_t)kZrViewRing + m.s.every - 1);
    } else if (f >= 2)
        ask(m, f - 2);      // (the head on the camera lane)
    m.pass.push_back(++m.tail);
    const bool rec = zr_end_records(m.s, f, args);
    if (rec) record(m, f);
    HOLDS(m.s.every != 1 || rec);                    // every = 1: every frame records, as before the rule
    HOLDS(rec || (args && m.s.prev_args && f % m.s.every != 0));
    m.sparse += !rec;
    zr_end_enqueued(&m.s, f, args, rec);
    m.frame_no++;
    if (m.print) printf("frame_no=%llu kind=%s recorded=%d\n", (unsigned long long)f, kKind[k], (int)rec);
}

// zr_finish, then zr_get_frame_periods over the last n frames: the runs tile the window, every frame of a run reports the same run, and
// the periods of a window whose ends are recorded sum to the time between the two records (time: the place in stream order).
static void periods(Model& m, uint64_t n)
{
    if (m.frame_no < 2) return;
    ask(m, m.frame_no - 1);
    if (n > m.frame_no - 1) n = m.frame_no - 1;
    if (n > (uint64_t)kZrEndRing - 1) n = kZrEndRing - 1;
    uint64_t top = m.frame_no - 1, sum_num = 0, lowest = top;
    bool whole = true;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t f = m.frame_no - 1 - k;
        uint64_t a = 0, b = 0;
        if (!zr_end_run(m.s, f, &a, &b)) { whole = false; break; }
        HOLDS(a < f && f <= b && b <= top && m.ev_frame[a % kZrEndRing] == a + 1 && m.ev_frame[b % kZrEndRing] == b + 1);
        HOLDS(m.ev_place[b % kZrEndRing] > m.ev_place[a % kZrEndRing]);      // (a period is > 0)
        if (f == b) { HOLDS(b == lowest); sum_num += m.ev_place[b % kZrEndRing] - m.ev_place[a % kZrEndRing]; lowest = a; }      // a run begins where the one above it ended
        else HOLDS(a == lowest);                                                                                              // ... and its other frames report it too
    }
    if (whole && n != 0 && m.frame_no - 1 - (n - 1) == lowest + 1)       // the window ends on a recorded end: exact
        HOLDS(sum_num == m.ev_place[top % kZrEndRing] - m.ev_place[lowest % kZrEndRing]);
    HOLDS(whole || n + m.s.every + 1 >= (uint64_t)kZrEndRing);      // (only a window as deep as the ring may reach out of it)
}

static void story()
{
    puts("== story");
    Model m; m.s.every = 4; m.print = true;
    for (int i = 0; i < 10; ++i) step(m, ONE_LAUNCH);
    step(m, ASK_LAST);                       // a texture update in the middle of the rest
    for (int i = 0; i < 3; ++i) step(m, ONE_LAUNCH);
    step(m, DRAWN); step(m, DRAWN);          // a camera cut: the first drawn frame's head asks for the end of the frame two before
    step(m, OTHER_REST); step(m, ONE_LAUNCH); step(m, ONE_LAUNCH);
    periods(m, 64);
    printf("story_broken %d\n", g_broken);
}

static void sweep(uint32_t every)
{
    unsigned long long sequences = 0, frames = 0, asks = 0, stand_ins = 0, recorded_now = 0, sparse = 0, paced = 0;
    const auto tally = [&](const Model& m) { ++sequences; frames += m.frame_no; asks += m.asks; stand_ins += m.stand_ins; recorded_now += m.recorded_now; sparse += m.sparse; paced += m.paced; };
    // every sequence of seven steps, behind a prefix of one-launch frames (and a drawn one) that ends just short of a turn of the ring
    static const int prefix[] = { 0, 5, kZrEndRing - 3, 2 * kZrEndRing - 5 };
    for (int pre : prefix) {
        Model base; base.s.every = every;
        for (int i = 0; i < pre; ++i) step(base, i == pre / 2 ? DRAWN : ONE_LAUNCH);
        int v[7] = { 0 };
        for (;;) {
            Model m = base;
            for (int i = 0; i < 7; ++i) step(m, (Kind)v[i]);
            periods(m, 16);
            tally(m);
            int i = 0;
            while (i < 7 && ++v[i] == KINDS) v[i++] = 0;
            if (i == 7) break;
        }
    }
    // one long sequence over several turns of the ring: rests of pseudo-random length, readers inside them, cuts between them
    Model m; m.s.every = every;
    uint32_t x = 12345u;
    const auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return x >> 16; };
    while (m.frame_no < 5u * kZrEndRing) {
        const uint32_t rest = 1u + rnd() % 40u;
        for (uint32_t i = 0; i < rest; ++i) { step(m, ONE_LAUNCH); if (rnd() % 9u == 0) step(m, rnd() % 2u ? ASK_LAST : ASK_BEFORE); }
        const uint32_t cut = rnd() % 4u;
        for (uint32_t i = 0; i < cut; ++i) step(m, rnd() % 3u ? DRAWN : OTHER_REST);
        if (rnd() % 7u == 0) periods(m, 1u + rnd() % 600u);
    }
    periods(m, 511);
    tally(m);
    printf("swept every=%u sequences=%llu frames=%llu asks=%llu stand_ins=%llu recorded_now=%llu sparse=%llu paced=%llu\n", every, sequences, frames, asks, stand_ins,
           recorded_now, sparse, paced);
}

int main()
{
    story();
    sweep(1); sweep(4); sweep(8);
    printf("broken %d\n", g_broken);
    return g_broken ? 1 : 0;
}
