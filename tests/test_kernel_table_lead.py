"""k_lighting_lead (csrc/zr_lighting.hip), the resting frame's launch that decides a part once, from the compiler's own listing (hipcc -S
for gfx950 with the library's flags, no GPU needed).

  - Its two instantiations (background off / on) are compiled for eight waves per SIMD: at most 64 VGPRs, no scratch.  Their rows - and
    nothing else - are recorded in profiles/r26_a_kernel_table_result.json (the file's other kernels are held to their own records by
    tests/test_kernel_table_stand.py, tests/test_kernel_table_rest.py and tests/test_kernel_table_rest_setup.py).
  - What the change is for: ahead of the first barrier - the decision, which k_lighting_stand makes in every wave - a wave that is not
    the workgroup's first issues a handful of instructions and no load.  The listing shows it as a branch over the decision ahead of
    every vector load of the kernel.
"""
import json
import os

from kernel_listing import ROOT, SRC, kernel_table, labels, listing, ops

RECORD = os.path.join(ROOT, "profiles", "r26_a_kernel_table_result.json")


def test_eight_waves_no_scratch_and_the_rows_are_the_recorded_ones():
    rows = kernel_table().table(SRC, [])
    want = json.load(open(RECORD))
    lead = {k: v for k, v in rows.items() if k.startswith("k_lighting_lead<")}
    assert sorted(lead) == ["k_lighting_lead<false, 512>", "k_lighting_lead<true, 512>"], sorted(rows)
    for name, r in lead.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr"] <= 64, (name, r)
    assert lead == {k: v for k, v in want.items() if k in lead}, lead


def test_the_other_waves_skip_the_decision_ahead_of_every_load(tmp_path):
    lines = listing(tmp_path, "k_lighting_lead<false, 512>")
    op, label = ops(lines), labels(lines)
    barrier = min(n for n, w in op if w[0] == "s_barrier")
    first_load = min(n for n, w in op if w[0].startswith("global_load"))
    skips = [(n, label[w[1]]) for n, w in op if w[0].startswith("s_cbranch") and n < first_load]
    print("first load at", first_load, "first barrier at", barrier, "branches ahead of the load", skips)
    assert skips, "no branch ahead of the first load"
    n, target = skips[0]
    between = [w[0] for k, w in op if target <= k < barrier]
    assert first_load < target <= barrier and not any(o.startswith("global_load") for o in between), between
    # what a sibling wave issues before it waits: a handful (its thread and wave numbers, an LDS address) where k_lighting_stand's
    # decision is 88 vector instructions
    assert len([w for k, w in op if k < n and w[0].startswith("v_")]) + len([o for o in between if o.startswith("v_")]) <= 8
