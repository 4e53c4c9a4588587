// settle_check.cpp — the generation rule of csrc/zr_settle.h without a GPU (tests/test_settle_rule.py builds and runs it, with the host
// sanitizers where g++ links them).
//
// A model of the target stands beside the rule.  Per part it holds what the kernel holds - a mark - and what only the model can know:
// whether the part's bytes in the target are still the lightless colour of the key they were written under (`good`).  Every sequence of
// frame kinds and key changes up to a length is swept; at every stand launch the kernel's skip condition (mark == gen, gen != 0) must
// imply `good`.  That is the statement "the generation never repeats across a frame that wrote the target by another kernel", checked as
// what it is for.  The other invariants are checked directly: two like frames share a generation, it is never 0 when on, the wrap wipes.
#include "zr_settle.h"

#include <cstdio>
#include <cstdlib>

enum Kind { STAND_SAME, STAND_NEW_KEY, OTHER_PASS, FORGET_THEN_STAND, KINDS };
static const char* kKind[KINDS] = { "stand", "stand_new_key", "other", "forget_stand" };

struct Model {
    ZrSettleState st;
    uint32_t mark = 0;       // one part no light reaches: the kernel marks it on every stand launch that shades it
    bool good = false;       // its bytes are the lightless colour of the current key
    uint32_t mark_lit = 0;   // a part some light has reached on every launch so far: never written lightless, so it may never stand
    uint32_t key = 0, launched_key = 0xFFFFFFFFu;
    long broken = 0, stands = 0, skips = 0, wipes = 0;
};

static void frame(Model& m, Kind k, bool print)
{
    if (k == STAND_NEW_KEY) { m.key++; m.good = false; }                     // another colour is due: what stands there is stale
    if (k == FORGET_THEN_STAND) { zr_settle_forget(&m.st); m.good = false; }   // (a background image replaced, the address handed out)
    ZrSettleFacts f;
    f.stand = k != OTHER_PASS;
    f.key_same = m.key == m.launched_key;
    const ZrSettleState before = m.st;
    const ZrSettleStep s = zr_settle_step(m.st, f);
    m.st = s.next;
    if (!f.stand) {
        m.good = false;                                                      // another kernel wrote the target
        if (s.gen != 0u || s.wipe || s.next.gen != before.gen || s.next.standing) m.broken++;
    } else {
        m.stands++;
        if (s.gen == 0u || s.gen != s.next.gen || !s.next.standing) m.broken++;                        // never 0 when on
        if (k == STAND_SAME && before.standing && before.gen != 0u && s.gen != before.gen) m.broken++;   // two like frames: one generation
        if (s.wipe) { m.mark = m.mark_lit = 0; m.wipes++; if (s.gen != 1u) m.broken++; }
        if (m.mark_lit == s.gen) m.broken++;                                 // (were its lights to leave now, it would be left alone)
        if (!s.wipe && s.gen < before.gen) m.broken++;                       // it only wraps behind a wipe
        if (m.mark == s.gen) { m.skips++; if (!m.good) m.broken++; }         // the kernel leaves the part alone: it must be good
        else { m.mark = s.gen; m.good = true; }                              // it shades the part and marks it
        m.launched_key = m.key;
    }
    if (print) printf("kind=%s gen=%u standing=%d wipe=%d mark=%u good=%d\n", kKind[k], s.gen, (int)s.next.standing, (int)s.wipe, m.mark, (int)m.good);
}

static long sweep(int len, uint32_t start_gen, Model* total)
{
    long n = 1;
    for (int i = 0; i < len; ++i) n *= KINDS;
    for (long code = 0; code < n; ++code) {
        Model m;
        m.st.gen = start_gen; m.mark_lit = start_gen ? 1u : 0u;
        long c = code;
        for (int i = 0; i < len; ++i) { frame(m, (Kind)(c % KINDS), false); c /= KINDS; }
        total->broken += m.broken; total->stands += m.stands; total->skips += m.skips; total->wipes += m.wipes;
    }
    return n;
}

int main()
{
    // a sequence written out, for the test to hold against the rule as DESIGN.md states it
    printf("== story\n");
    Model m;
    const Kind story[] = { OTHER_PASS, OTHER_PASS, STAND_SAME, STAND_SAME, STAND_SAME, STAND_NEW_KEY, STAND_SAME, OTHER_PASS, STAND_SAME, STAND_SAME,
                           FORGET_THEN_STAND, STAND_SAME };
    for (Kind k : story) frame(m, k, true);
    printf("story_broken %ld\n", m.broken);

    // the wrap: the generation before the wrap, a mark of generation 1 left from 2^32 launches ago
    printf("== wrap\n");
    Model w;
    w.st.gen = 0xFFFFFFFEu; w.mark = 1u; w.mark_lit = 1u; w.good = false;
    const Kind wrap[] = { STAND_SAME, STAND_SAME, OTHER_PASS, STAND_SAME, STAND_SAME, OTHER_PASS, STAND_SAME };
    for (Kind k : wrap) frame(w, k, true);
    printf("wrap_broken %ld wipes %ld\n", w.broken, w.wipes);

    Model total;
    const long a = sweep(8, 0u, &total), b = sweep(7, 0xFFFFFFFCu, &total);
    printf("swept %ld %ld stands %ld skips %ld wipes %ld\n", a, b, total.stands, total.skips, total.wipes);
    printf("broken %ld\n", total.broken);
    return total.broken == 0 && m.broken == 0 && w.broken == 0 ? 0 : 1;
}
