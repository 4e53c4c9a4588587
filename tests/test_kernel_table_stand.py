"""k_lighting_stand (csrc/zr_lighting.hip), the resting frame's launch that leaves settled parts alone, from the compiler's own listing
(hipcc -S for gfx950 with the library's flags, no GPU needed).

  - Its two instantiations (background off / on; the tile list is always built, as a ballot) are compiled for eight waves per SIMD: at
    most 64 VGPRs, no scratch.  Their rows - and nothing else - are recorded in profiles/r26_a_kernel_table_result.json (the other
    kernels of the file are held to their own records by tests/test_kernel_table_rest.py and tests/test_kernel_table_rest_setup.py).
  - The returning path - a part no point light reaches, whose mark stands - leaves ahead of the workgroup's first barrier: the branch
    that takes it sits behind ONE trip of three vector loads (the part's records, the two halves of the lane's light record; the mark
    is a scalar load beside them), ahead of every table load, and the block it goes to lies behind the kernel's last s_barrier and
    runs to s_endpgm: no barrier is met on the way.  A part that shades updates its mark BEHIND the set-up's barrier - every wave of
    the workgroup has read the mark by then, so none can see its own launch's store and return: no store sits ahead of it.  The same source built with -DZR_STAND_EARLY_EXIT=0 - everything in one trip, the
    exit behind the set-up's barrier: the order that lost, DESIGN.md App. A - has the table loads ahead of that branch and exactly one
    barrier, the set-up's, between the kernel's entry and it.
"""
import json
import os

from kernel_listing import ROOT, SRC, kernel_table, labels, listing, ops

KERNEL = "k_lighting_stand<false, 512>"
RECORD = os.path.join(ROOT, "profiles", "r26_a_kernel_table_result.json")


def _listing(tmp, extra=()):
    return listing(tmp, KERNEL, extra)


def _exit_path(lines):
    """-> (line of the branch that takes the returning path, line of its target's label, lines of every s_barrier, of s_endpgm)"""
    op = ops(lines)
    barriers = [n for n, w in op if w[0] == "s_barrier"]
    ends = [n for n, w in op if w[0] == "s_endpgm"]
    assert len(ends) == 1, ends
    label = labels(lines)
    # the conditional branches ahead of the kernel's last barrier (the empty colour's) whose target lies behind it: the returning path is
    # the first such jump (the others, late in the kernel, are those of a part that shades and holds no empty pixel)
    out = [(n, label[w[1]]) for n, w in op if w[0].startswith("s_cbranch") and n < barriers[-1] and label[w[1]] > barriers[-1]]
    assert out and len(barriers) == 2, (out, barriers)
    return out[0][0], out[0][1], barriers, ends[0]


def _loads_before(lines, n):
    return [l.split()[0] for l in lines[:n] if l.strip().startswith("global_load")]


def test_eight_waves_no_scratch_and_the_rows_are_the_recorded_ones():
    rows = kernel_table().table(SRC, [])
    want = json.load(open(RECORD))
    stand = {k: v for k, v in rows.items() if k.startswith("k_lighting_stand<")}
    assert sorted(stand) == ["k_lighting_stand<false, 512>", "k_lighting_stand<true, 512>"], sorted(rows)
    for name, r in stand.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr"] <= 64, (name, r)
    assert stand == {k: v for k, v in want.items() if k in stand}, stand


def test_the_returning_path_meets_no_barrier(tmp_path):
    lines = _listing(tmp_path)
    branch, target, barriers, end = _exit_path(lines)
    print("branch at", branch, "first barrier at", barriers[0], "target at", target, "last barrier at", barriers[-1], "end at", end)
    assert branch < barriers[0] and barriers[-1] < target < end
    loads = _loads_before(lines, branch)
    assert sorted(loads) == ["global_load_dword", "global_load_dwordx4", "global_load_dwordx4"], loads      # records, the light's two halves
    waits = [n for n, l in enumerate(lines[:branch]) if l.split()[:1] == ["s_waitcnt"] and "vmcnt" in l]
    last_load = max(n for n, l in enumerate(lines[:branch]) if l.strip().startswith("global_load"))
    assert waits and min(waits) > last_load, (waits, last_load)      # one trip: all three are requested before the first is waited for
    stores = [n for n, l in enumerate(lines[:barriers[0]]) if l.strip().startswith("global_store")]
    assert not stores, stores      # the mark's update (and every other store of a part that shades) lies behind the set-up's barrier


def test_the_other_order_exits_behind_the_set_ups_barrier(tmp_path):
    lines = _listing(tmp_path, ["-DZR_STAND_EARLY_EXIT=0"])
    branch, target, barriers, end = _exit_path(lines)
    print("branch at", branch, "barriers at", barriers, "target at", target)
    assert len([b for b in barriers if b < branch]) == 1 and barriers[-1] < target < end
    assert len(_loads_before(lines, branch)) == 6      # ... and the three of the tables
