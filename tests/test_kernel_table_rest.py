"""The one-launch resting frame's kernels, and the kernels it must leave alone, from the compiler's own report (tools/kernel_table.py:
hipcc -S for gfx950, no GPU needed).

k_lighting_rest (csrc/zr_lighting.hip) takes its uniforms by argument and indexes the argument's light records by a wave-uniform index:
that must stay scalar loads, not a private copy of the argument - no scratch - and the kernel is compiled for eight waves per SIMD:
at most 64 VGPRs.  The lighting kernels that keep nothing (k_lighting<..., 0>) and the forward variant share their device functions
with it (csrc/zr_shade.h): their rows - registers, scratch, LDS, instruction counts - are the rows of the commit before the change,
as recorded with that commit in profiles/r14_a_kernel_table_result.json.
"""
import json
import os

import pytest

from kernel_listing import ROOT, kernel_table


@pytest.fixture(scope="module")
def rows():
    kt = kernel_table()
    out = {}
    for src in ("zr_lighting.hip", "zr_forward.hip"):
        out.update(kt.table(os.path.join(ROOT, "zeldaengine_amd", "csrc", src), []))
    return out


def test_by_argument_kernels_hold_eight_waves_without_scratch(rows):
    rest = {k: v for k, v in rows.items() if k.startswith("k_lighting_rest<")}
    assert len(rest) == 4, sorted(rows)          # tile light list on / off x background on / off
    for name, r in rest.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr"] <= 64, (name, r)


def test_plain_and_forward_rows_are_the_parents(rows):
    table = json.load(open(os.path.join(ROOT, "profiles", "r14_a_kernel_table_result.json")))
    parent = {k: v for k, v in table.items() if k.startswith("k_forward<") or (k.startswith("k_lighting<") and k.endswith(", 0u>"))}
    assert len(parent) == 6, sorted(parent)
    for name, was in parent.items():
        assert rows.get(name) == was, (name, rows.get(name), was)
