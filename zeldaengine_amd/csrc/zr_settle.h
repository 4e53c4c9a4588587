// zr_settle.h — when the pixels a resting frame's launch leaves alone can be vouched for ("The schedule";
// k_lighting_stand in zr_lighting.hip).  A part's mark says "this part's pixels in the target are the colour no point light feeds, written
// under generation g"; it stands only while g is the current generation.  zr_settle_step() is the whole rule: the state the lighting passes
// so far left + what this pass is -> the generation this pass runs under.  Plain C++17 and nothing of HIP, like zr_frame_plan.h:
// tests/settle_check.cpp compiles this header alone and sweeps it without a GPU.
#pragma once

#include <cstdint>

// What the lighting passes enqueued so far left behind.  gen: the generation the marks were last written under (0: none yet).  standing:
// the pass enqueued last was a k_lighting_stand launch under `gen`, and nothing since can have changed the settled colour or the target's
// bytes (zr_settle_forget clears it: the calls that change what light_emit reads without a drawn frame, or hand the target out).
struct ZrSettleState { uint32_t gen = 0; bool standing = false; };

// This lighting pass.  stand: it is a k_lighting_stand launch on a context that may settle (false: any other pass - plain, fill, kept
// through XkView, forward, view 9, a demoted frame, k_lighting_rest).  key_same: the byte image of what the settled colour and its
// address depend on - the pass's parameters without the next map's clear, the camera, the directional count, the target, the plane, the
// records, the owned tiles and their count, the marks - is the previous stand launch's, compared by the caller.
struct ZrSettleFacts { bool stand = false, key_same = false; };

// gen: what the launch is given (0: nothing settles, nothing is marked - every pass that is not a stand launch).  wipe: the generation
// wrapped, and the marks are zero-filled ahead of the launch (a mark of 2^32 launches ago would otherwise stand again).
struct ZrSettleStep { ZrSettleState next; uint32_t gen = 0; bool wipe = false; };

static inline ZrSettleStep zr_settle_step(const ZrSettleState& before, const ZrSettleFacts& f)
{
    ZrSettleStep s;
    s.next = before;
    if (!f.stand) { s.next.standing = false; return s; }      // the target was written by another kernel: the next stand launch moves on
    if (!before.standing || !f.key_same || before.gen == 0u) {
        s.next.gen = before.gen + 1u;
        if (s.next.gen == 0u) { s.next.gen = 1u; s.wipe = true; }
    }
    s.next.standing = true;
    s.gen = s.next.gen;
    return s;
}
// Something changed the settled colour or the target behind the kernel's back.
static inline void zr_settle_forget(ZrSettleState* s) { s->standing = false; }
