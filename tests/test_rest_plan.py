"""The one-launch resting frame in the schedule, without a GPU (csrc/zr_frame_plan.h: ZrFrameFacts::light_by_arg, ZrFramePlan::light_args).

tests/rest_plan_check.cpp compiles tests/frame_plan_check.cpp into itself as it stands and runs its sweeps and every invariant of its
check() twice over a context whose lighting pass keeps - light_by_arg off, then on - plus the invariants of the new flag; it is built
stand-alone, with the address and undefined-behaviour sanitizers where this machine's g++ links them.  What its sequences must print is
written out below from the rule ("The schedule"), not from the program: a frame that reads the plane and may take
its uniforms by argument is one launch on the host's stream - no head on the lane, no one-pixel launch, no event; a frame that fills
the plane keeps its head on the host's stream, because its one-pixel launch writes the slot the frame before may still be reading.
"""
import math
import os
import subprocess

import pytest

from test_frame_plan import SWEEPS, VALUES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

ONE_LAUNCH = "map=kept pass=whole shadow=none camera=none resolve=none head=host one_pixel=none lighting=host ev_cam=none host_waits=0 " \
             "wait_end2=0 wait_end1=0 wait_lane_end=0 wait_ids=0 reset_stats=0 reset_list=0"
FILL = "map=kept pass=whole shadow=none camera=none resolve=none head=host one_pixel=host lighting=host ev_cam=none host_waits=0 wait_end2=0"
ON_LANE = "map=kept pass=whole shadow=none camera=none head=cam one_pixel=cam ev_cam=one_pixel host_waits=1 wait_end2=1"


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """{by_arg: {"sequences": {name: rows}, "swept": {name: n}, "broken": n}}, "rest_seen": {...}, "rest_broken": n"""
    d = tmp_path_factory.mktemp("rest_plan")
    hello = d / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    sanitize = SANITIZE if subprocess.call(["g++"] + SANITIZE + [str(hello), "-o", str(d / "hello")], stderr=subprocess.DEVNULL) == 0 and \
        subprocess.call([str(d / "hello")]) == 0 else []
    exe = d / "rest_plan_check"
    subprocess.check_call(["g++"] + FLAGS + sanitize + ["-I", CSRC, "-I", os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "rest_plan_check.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    out, cur, name = {}, None, None
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "rest":
            cur = out.setdefault(int(w[1].split("=")[1]), {"sequences": {}, "swept": {}, "broken": None})
        elif w[0] == "==":
            name = w[1]
            cur["sequences"][name] = []
        elif w[0].startswith("frame="):
            cur["sequences"][name].append(dict(x.split("=") for x in w))
        elif w[0] == "swept":
            cur["swept"][w[1]] = int(w[2])
        elif w[0] == "broken":
            cur["broken"] = int(w[1])
        elif w[0] == "rest_seen":
            out["rest_seen"] = {k: int(v) for k, v in (x.split("=") for x in w[1:])}
        elif w[0] == "rest_broken":
            out["rest_broken"] = int(w[1])
    return out


def holds(rows, expected, first=0):
    assert len(rows) == len(expected)
    for n, (row, want) in enumerate(zip(rows, expected), first):
        assert row["frame"] == str(n)
        for word in want.split():
            k, v = word.split("=")
            assert row[k] == v, "frame %d: %s is %s, not %s" % (n, k, row[k], v)


def test_a_rest_is_one_launch_from_the_frame_after_the_fill(report):
    """Frames 0 and 1 draw, frame 2 rests and fills, on the host's stream; from frame 3 the frame is the one launch - or, where the
    uniforms may not travel by argument, as before: head and one-pixel launch on the idle lane."""
    drawn = ["map=drawn head=cam one_pixel=host", "map=kept pass=two_rounds head=cam one_pixel=host"]
    holds(report[1]["sequences"]["rest_render"], drawn + [FILL] + [ONE_LAUNCH] * 5)
    holds(report[0]["sequences"]["rest_render"], drawn + [FILL] + [ON_LANE] * 5)


def test_staged_entry_points_rest_the_same_way(report):
    drawn = ["map=drawn head=host one_pixel=host", "map=kept pass=two_rounds head=host one_pixel=host"]
    holds(report[1]["sequences"]["rest_staged"], drawn + [FILL + " ev_join=1"] + [ONE_LAUNCH + " ev_join=1"] * 5)
    holds(report[0]["sequences"]["rest_staged"], drawn + [FILL + " ev_join=1"] + ["pass=whole head=host one_pixel=host ev_cam=none ev_join=1"] * 5)


def test_a_light_that_stops(report):
    """The light's last move is frame 4: frames 2 - 4 keep the camera pass but draw the map - no rest, nothing by argument; frame 5 fills;
    frames 6 and 7 are one launch."""
    moving = "map=drawn pass=whole shadow=host head=host one_pixel=host"
    holds(report[1]["sequences"]["light_stops"], ["map=drawn"] * 2 + [moving] * 3 + [FILL] + [ONE_LAUNCH] * 2)
    holds(report[0]["sequences"]["light_stops"], ["map=drawn"] * 2 + [moving] * 3 + [FILL] + [ON_LANE] * 2)


def test_only_a_context_with_the_slot_fills_with_its_head_on_the_hosts_stream(report):
    """The plane is forgotten in the middle of a rest, where a resting frame's head is on the lane: frame 5 fills again.  With the slot
    its head goes to the host's stream for that frame (the one-pixel launch writes the slot); without it (no room, or a build with
    several pixels per thread) nothing can race and the head stays on the lane, as before the slot existed."""
    holds(report[0]["sequences"]["refill_slot"][3:], [ON_LANE, ON_LANE, FILL, ON_LANE, ON_LANE], first=3)
    holds(report[0]["sequences"]["refill_no_slot"][3:], [ON_LANE] * 5, first=3)


def test_invariants_hold_with_the_fact_on_and_off(report):
    """Every invariant of frame_plan_check.cpp's check() and those of the new flag, over every combination of each sweep's dimensions,
    twice; plans that were one launch, that read and that filled were all met."""
    assert report["rest_broken"] == 0
    for by_arg in (0, 1):
        assert report[by_arg]["broken"] == 0
        for name, dims in SWEEPS.items():
            assert report[by_arg]["swept"][name] == math.prod(VALUES[d] for d in dims), (by_arg, name)
    seen = report["rest_seen"]
    assert seen["light_keep"] > seen["light_args"] > 0 and seen["light_fill"] > 0, seen
