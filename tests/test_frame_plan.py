"""The frame schedule without a GPU (csrc/zr_frame_plan.h: zr_frame_plan, zr_frame_carry).

tests/frame_plan_check.cpp includes the header alone - plain C++17, nothing of HIP - and is compiled and run here, with the address and
undefined-behaviour sanitizers where this machine's g++ links them for a stand-alone program.  It drives the two functions through
scripted sequences of frames, one printed line per frame, and holds the schedule's invariants over every combination of the facts it
sweeps.  What the sequences must print is written out below, from DESIGN.md section 5 "The schedule" and the docstrings of
tests/test_gpu_shadow_keep.py, test_gpu_round2_keep.py, test_gpu_gbuffer_keep.py and test_gpu_resolve_lane.py - not from the program.
"""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """The program's output: {"sequences": {name: [ {key: value} per frame ]}, "swept": {name: combinations}, "seen": {...}, "broken": n}."""
    d = tmp_path_factory.mktemp("frame_plan")
    hello = d / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    sanitize = SANITIZE if subprocess.call(["g++"] + SANITIZE + [str(hello), "-o", str(d / "hello")], stderr=subprocess.DEVNULL) == 0 and \
        subprocess.call([str(d / "hello")]) == 0 else []
    exe = d / "frame_plan_check"
    subprocess.check_call(["g++"] + FLAGS + sanitize + ["-I", CSRC, os.path.join(ROOT, "tests", "frame_plan_check.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    out = {"sequences": {}, "swept": {}, "seen": {}, "broken": None, "sanitized": bool(sanitize)}
    name = None
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "==":
            name = w[1]
            out["sequences"][name] = []
        elif w[0].startswith("frame="):
            out["sequences"][name].append(dict(x.split("=") for x in w))
        elif w[0] == "swept":
            out["swept"][w[1]] = int(w[2])
        elif w[0] == "seen":
            out["seen"] = {k: int(v) for k, v in (x.split("=") for x in w[1:])}
        elif w[0] == "broken":
            out["broken"] = int(w[1])
    return out


def holds(report, name, expected):
    """expected: per frame a string of key=value words the frame's line must carry."""
    rows = report["sequences"][name]
    assert len(rows) == len(expected), (name, len(rows))
    for n, (row, want) in enumerate(zip(rows, expected)):
        assert row["frame"] == str(n)
        for word in want.split():
            k, v = word.split("=")
            assert row[k] == v, "%s, frame %d: %s is %s, not %s" % (name, n, k, row[k], v)


# Words for what a frame does.  All of it on the host's stream: no event between lanes, ev_join recorded.
ONE_STREAM = "head=host lighting=host ev_cam=none host_waits=0 wait_end2=0 wait_end1=0 wait_ids=0 ev_join=1 one_pixel=host"
# first frame of a scene: no history, no plan - one round, k_geom counts first; the map is drawn
FIRST = "map=drawn pass=one_round count_first=1 plan_rounds=0 reset_stats=1"
# a zr_render frame on two lanes that draws its map: camera pipeline and resolve on the lane, ev_cam at the lane's end
LANE = "head=cam shadow=host camera=cam resolve=cam deferred=0 one_pixel=host lighting=host ev_cam=lane_end host_waits=1 ev_join=0"
# ... that keeps its map: the resolve on the host's stream, ev_cam behind k_mark
MOVED = "head=cam shadow=none map=kept camera=cam resolve=host deferred=1 one_pixel=host lighting=host ev_cam=mark host_waits=1 ev_join=0"
# camera pass kept whole and map kept, for a frame already: upload and one-pixel launch on the idle lane
RESTING = "map=kept pass=whole shadow=none camera=none resolve=none deferred=0 head=cam one_pixel=cam ev_cam=one_pixel host_waits=1 reset_stats=0 reset_list=0 wait_end1=0 wait_lane_end=0"
# camera pass kept whole, head on the host's stream: nothing on the lane, nothing to wait for
WHOLE_ON_HOST = "pass=whole camera=none resolve=none deferred=0 head=host one_pixel=host ev_cam=none host_waits=0 reset_stats=0 wait_end2=0 wait_end1=0"


def test_resting_zr_render_on_two_lanes(report):
    holds(report, "rest_render", [FIRST + " " + LANE + " wait_end2=0",
                                  "pass=two_rounds count_first=0 plan_rounds=1 " + MOVED + " wait_end2=0"] + [RESTING + " wait_end2=1"] * 6)


@pytest.mark.parametrize("name", ["rest_serial", "rest_staged"])
def test_resting_on_one_stream_keeps_the_same_and_crosses_no_lane(report, name):
    drawn = " shadow=host camera=host resolve=host deferred=0 " + ONE_STREAM
    holds(report, name, [FIRST + drawn, "map=kept pass=two_rounds count_first=0 shadow=none camera=host resolve=host deferred=0 " + ONE_STREAM] +
          ["map=kept pass=whole shadow=none camera=none resolve=none deferred=0 reset_stats=0 " + ONE_STREAM] * 6)


def test_camera_cut(report):
    """Frames k and k + 1 draw two rounds (k's history is the old view's: round 2 is not kept on it), k + 2 keeps whole."""
    cut = "pass=two_rounds count_first=0 " + MOVED
    holds(report, "camera_cut", [FIRST, "pass=two_rounds", RESTING, RESTING, cut, cut, RESTING, RESTING])


def test_texture_update(report):
    """A surface-only change: round 2 stays kept, but both GBuffer copies are resolved again before the pass is kept whole."""
    again = "pass=round2_kept plan_rounds=2 count_first=0 " + MOVED
    holds(report, "texture_update", [FIRST, "pass=two_rounds", RESTING, RESTING, again, again, RESTING, RESTING])


def test_moving_light(report):
    """The map is drawn every frame; the camera pass is kept whole all the same, with its head where the frame is lit."""
    holds(report, "light_moves", [FIRST + " " + LANE, "map=drawn pass=two_rounds " + LANE] + ["map=drawn shadow=host " + WHOLE_ON_HOST] * 6)


def test_light_stops(report):
    """The light's last move is frame 4: frame 5 keeps the map, but frame 4 drew it on the host's stream, behind nothing the lane has waited
    for - the head goes to the lane from frame 6."""
    holds(report, "light_stops", ["map=drawn"] * 2 + ["map=drawn shadow=host " + WHOLE_ON_HOST] * 3 + ["map=kept shadow=none " + WHOLE_ON_HOST] +
          [RESTING + " wait_end2=1"] * 2)


def test_scene_edit_starts_over(report):
    """zr_scene_finalize forgets history, plan and lists and changes the casters: the next frame is a first frame."""
    holds(report, "scene_edit", [FIRST + " " + LANE, "pass=two_rounds " + MOVED, RESTING, RESTING,
                                 FIRST + " " + LANE + " wait_end2=1", "pass=two_rounds " + MOVED, RESTING, RESTING])


def test_no_list_reuse_keeps_nothing(report):
    every = "map=drawn shadow_list=rebuilt camera_list=rebuilt reset_list=1 " + LANE
    holds(report, "no_list_reuse", [every + " pass=one_round"] + [every + " pass=two_rounds plan_rounds=1"] * 7)


def test_no_hiz_draws_one_round(report):
    holds(report, "no_hiz", [FIRST + " hiz=0 " + LANE] + ["pass=one_round hiz=0 count_first=0 plan_rounds=0 " + MOVED] * 7)


def test_tile_partitioned_context(report):
    """The host gathers a partitioned map in place: never kept.  The camera pass is kept like anywhere else; the lists stand."""
    holds(report, "tile_world_2", [FIRST + " shadow_list=rebuilt camera_list=rebuilt reset_list=1 " + LANE,
                                   "map=drawn pass=two_rounds shadow_list=reused camera_list=reused reset_list=0 " + LANE] +
          ["map=drawn shadow=host shadow_list=reused " + WHOLE_ON_HOST] * 6)


def test_skydome(report):
    """The sky key plane is single-buffered: round 2 is kept, the pass never whole, the resolve never leaves the lane."""
    holds(report, "skydome", [FIRST + " " + LANE, "map=kept pass=two_rounds resolve=cam deferred=0 ev_cam=lane_end"] +
          ["map=kept pass=round2_kept plan_rounds=2 camera=cam resolve=cam deferred=0 head=cam ev_cam=lane_end host_waits=1 reset_stats=1"] * 6)


def test_lane_hand_over(report):
    """Frame 1 resolved on the host's stream: its ev_cam sat ahead of the lane's k_plan, so the staged frame 2 (drawn: the camera moved) waits
    for the lane's end.  Frame 3 is on the lane again, behind a camera pipeline on the host's stream: it waits for ev_end[2]."""
    holds(report, "lane_handover", [LANE, MOVED + " wait_lane_end=0",
                                    "pass=two_rounds camera=host resolve=host deferred=0 wait_lane_end=1 " + ONE_STREAM,
                                    "pass=two_rounds wait_end1=1 wait_end2=1 wait_lane_end=0 " + MOVED])


# What the three sweeps take every combination of, and how many values each dimension has (frame_plan_check.cpp: enum Dim, kValues).
VALUES = {"NO_HIZ": 2, "SERIAL": 2, "NO_LIST_REUSE": 2, "SHADOW_OCCLUSION": 2, "NO_SHADOW_OCCLUSION": 2,
          "PARTITION": 4,            # none, the frame's tiles, the casters' instances, the map's tiles
          "MAP_EXTERNAL": 2, "SKY": 2, "FORWARD": 2,
          "ENTRY": 3,                # zr_render, zr_render_geometry, zr_render_shadow
          "HAS_LANE": 2, "FRAME_NO": 4, "SHADOW_IS_MAP": 2, "CAMERA_IS_PREV": 2, "CASTER_EPOCH": 2, "CAMERA_EPOCH": 2, "SURFACE_EPOCH": 2,
          "SHADOW_LIST": 3, "CAMERA_LIST": 3,      # no list, built from this block, built from another
          "N_WORK_SHADOW": 2, "N_WORK_CAMERA": 2,
          "COPY_GEN": 4, "COPY_OVERLAY": 4, "COPY_IDS_WAIT": 4,      # per GBuffer copy
          "SMAP_VALID": 2, "SMAP_AGE": 2, "CAM_PREV_VALID": 2, "R2_SETTLED": 2, "PLAN_VALID": 2, "PLAN_TWO_ROUND": 2, "VIS_HISTORY": 2,
          "LIST_VALID_SHADOW": 2, "LIST_VALID_CAMERA": 2, "PLAN_BEHIND_CAM": 2,
          "GBUF_LANE": 3,            # none yet, the host's stream, the lane
          "SFLAG_HISTORY": 2}
SWEEPS = {
    "shadow": ["NO_LIST_REUSE", "SHADOW_OCCLUSION", "NO_SHADOW_OCCLUSION", "PARTITION", "MAP_EXTERNAL", "SERIAL", "ENTRY", "HAS_LANE", "FRAME_NO",
               "SHADOW_IS_MAP", "CASTER_EPOCH", "SHADOW_LIST", "N_WORK_SHADOW", "SMAP_VALID", "SMAP_AGE", "LIST_VALID_SHADOW", "SFLAG_HISTORY"],
    "camera": ["NO_HIZ", "NO_LIST_REUSE", "SKY", "CAMERA_IS_PREV", "CAMERA_EPOCH", "SURFACE_EPOCH", "CAMERA_LIST", "N_WORK_CAMERA", "COPY_GEN",
               "COPY_OVERLAY", "SMAP_VALID", "CAM_PREV_VALID", "R2_SETTLED", "PLAN_VALID", "PLAN_TWO_ROUND", "VIS_HISTORY", "LIST_VALID_CAMERA"],
    "lanes": ["SERIAL", "SKY", "FORWARD", "ENTRY", "HAS_LANE", "FRAME_NO", "COPY_GEN", "COPY_IDS_WAIT", "SMAP_VALID", "SMAP_AGE", "R2_SETTLED",
              "PLAN_VALID", "VIS_HISTORY", "PLAN_BEHIND_CAM", "GBUF_LANE"],
}


def test_invariants_hold_over_every_combination(report):
    """The program exits 0 only if no invariant broke (the fixture asserts the exit status); it visited every combination of each sweep's
    dimensions - a dimension dropped from a loop changes the product - every dimension is in some sweep, and every regime the invariants
    speak of was met."""
    assert report["broken"] == 0
    for name, dims in SWEEPS.items():
        assert report["swept"][name] == math.prod(VALUES[d] for d in dims), name
    assert report["swept"]["all"] == sum(math.prod(VALUES[d] for d in dims) for dims in SWEEPS.values())
    assert set().union(*SWEEPS.values()) == set(VALUES)
    assert all(n > 0 for n in report["seen"].values()) and len(report["seen"]) == 5, report["seen"]
