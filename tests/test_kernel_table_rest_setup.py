"""How k_lighting_rest sets its part up, from the compiler's own listing (hipcc -S for gfx950 with the library's flags, no GPU needed).

The eight records of a workgroup's part (csrc/zr_types.h: ZrRestRecord) used to be read by a loop - a scalar load and a wait per record;
now they arrive as one vector load per lane behind one wait, and the box is folded on the DPP network.  A light's record arrives whole:
one 32-byte scalar load in the light loop, two 16-byte LDS reads for the tile list's test.  The table floats, the light records' LDS
copy and the part's records are requested before the first of them is waited for.

The listing is held to that, for k_lighting_rest<true, false, 512>:
  - the kernel has two loops - the next map's clear and the walk over the tile's light list - and the same listing built with
    -DZR_REST_RECORDS_ONE_TRIP=0, the records' loop put back, has three: the test can tell them apart;
  - between the workgroup's barrier and the first DPP instruction the records are waited for once, and the fold is six row_shr steps;
  - the light loop holds one scalar load, of eight dwords; the tile list's test reads its light by two 16-byte LDS reads side by side;
  - ahead of the barrier five loads - three of tables, the light records, the part's records - are issued before the first wait on one.
The instruction counts tools/kernel_table.py reports for the four instantiations are recorded in profiles/r26_a_kernel_table_result.json;
the table the tool makes now is that file's (registers, scratch and LDS included: at most 64 VGPRs, no scratch).
"""
import json
import os
import re

import pytest

from kernel_listing import ROOT, SRC, kernel_table, listing as kernel_listing, ops

KERNEL = "k_lighting_rest<true, false, 512>"


def _listing(tmp, extra=()):
    """the instruction lines (comments kept) of KERNEL"""
    return kernel_listing(tmp, KERNEL, extra)


def _loops(lines):
    """[(line number of the header, depth, labels of its child loops)] from the compiler's loop comments"""
    out = []
    for n, line in enumerate(lines):
        m = re.search(r"; =>This (Inner )?Loop Header: Depth=(\d+)", line)
        if m:
            kids = []
            for nxt in lines[n + 1:]:
                k = re.match(r"\s*;\s+Child Loop (\S+) Depth (\d+)", nxt)
                if not k:
                    break
                kids.append((k.group(1), int(k.group(2))))
            out.append((n, int(m.group(2)), kids))
    return out


def _ops(lines):
    return [(n, w[0], lines[n]) for n, w in ops(lines) if not w[0].endswith(":")]


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    return _listing(tmp_path_factory.mktemp("rest_setup"))


def _barrier(ops):
    return next(i for i, o in enumerate(ops) if o[1] == "s_barrier")


def test_no_loop_over_the_records(listing, tmp_path):
    loops = _loops(listing)
    print(loops)
    assert len(loops) == 2 and all(l[1] == 1 and not l[2] for l in loops), loops
    back = _loops(_listing(tmp_path, ["-DZR_REST_RECORDS_ONE_TRIP=0"]))
    assert len(back) == 3, back


def test_one_wait_for_a_parts_records(listing):
    ops = _ops(listing)
    ops = ops[_barrier(ops):]
    dpp = next(i for i, o in enumerate(ops) if "row_shr" in o[2])
    waits = [o[2].strip() for o in ops[:dpp] if o[1] == "s_waitcnt" and "vmcnt" in o[2]]
    print(waits)
    assert len(waits) == 1, waits
    assert not [o for o in ops[:dpp] if o[1].startswith("global_load")]      # (requested ahead of the barrier, with the tables)
    assert len([o for o in ops[dpp:dpp + 60] if "row_shr" in o[2]]) == 6      # min and max over eight lanes: three steps each


def _blocks_of(lines, label):
    """the lines of every basic block the compiler marks as part of the loop headed by `label` (BBn_m), the header's own included"""
    out, inside = [], False
    for line in lines:
        if re.match(r"\.LBB\S+:", line):
            inside = line.startswith(".L" + label + ":") or ("in Loop: Header=" + label + " ") in line
        elif inside:
            out.append(line)
    return out


def test_a_light_record_arrives_whole(listing):
    labels = [re.match(r"\.L(BB\S+):", listing[n]).group(1) for n, _, _ in _loops(listing)]
    loads = [[l.split()[0] for l in _blocks_of(listing, label) if l.strip().startswith("s_load")] for label in labels]
    print(loads)
    assert sorted(loads) == [[], ["s_load_dwordx8"]], loads      # the clear's loop loads nothing; the light loop one record
    ops = _ops(listing)
    reads = [i for i, o in enumerate(ops) if o[1] == "ds_read_b128"]
    assert len(reads) == 2 and reads[1] == reads[0] + 1, [ops[i][2] for i in reads]


def test_the_tables_arrive_in_one_trip(listing):
    ops = _ops(listing)
    before = ops[:_barrier(ops)]
    loads = [i for i, o in enumerate(before) if o[1].startswith("global_load")]
    first_wait = next(i for i, o in enumerate(before) if o[1] == "s_waitcnt" and "vmcnt" in o[2])
    print(len(loads), "loads,", "first wait on one after", first_wait, "instructions")
    assert len(loads) == 5 and max(loads) < first_wait, [before[i][2] for i in loads]


def test_instruction_counts_are_the_recorded_ones():
    rows = {k: v for k, v in kernel_table().table(SRC, []).items() if k.startswith("k_lighting_rest<")}
    want = json.load(open(os.path.join(ROOT, "profiles", "r26_a_kernel_table_result.json")))
    assert len(rows) == 4 and rows == {k: v for k, v in want.items() if k.startswith("k_lighting_rest<")}, rows
    for name, r in rows.items():
        assert r["scratch"] == 0 and r["vgpr"] <= 64, (name, r)
