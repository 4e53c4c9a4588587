"""The end-of-frame event recorded where someone will ask for it, without a GPU (csrc/zr_frame_end.h).

tests/frame_end_check.cpp is built stand-alone, with the address and undefined-behaviour sanitizers where this machine's g++ links them.
It runs the rule beside a model of the host's stream that knows what the state only claims - where in stream order every lighting pass
and every record really sits, and which frame each slot's event was really recorded for - over every sequence of seven steps drawn from:
a frame of one launch, another resting frame, a drawn frame, a reader asking for the end of the frame enqueued last, or of the one
before; begun at frame 0 and just short of a turn of the 512-slot ring; and over one long sequence of five turns; with every = 1, 4, 8.
What it checks, from the rule ("The schedule"):
  - the event handed to a reader was recorded behind the asked frame's lighting pass, and its slot holds the frame the state says;
  - a one-launch frame leaves the host at most VIEW_RING + every - 1 frames ahead of the newest end it synchronised on;
  - every = 1: every frame records its end;
  - the reported periods are run means: the runs tile the window, and a window whose ends are recorded sums to the time between them.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame_end")
    hello = d / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    sanitize = SANITIZE if subprocess.call(["g++"] + SANITIZE + [str(hello), "-o", str(d / "hello")], stderr=subprocess.DEVNULL) == 0 and \
        subprocess.call([str(d / "hello")]) == 0 else []
    exe = d / "frame_end_check"
    subprocess.check_call(["g++"] + FLAGS + sanitize + ["-I", CSRC, os.path.join(ROOT, "tests", "frame_end_check.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    out = {"story": [], "swept": {}}
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0].startswith("frame_no="):
            out["story"].append(dict(x.split("=") for x in w))
        elif w[0] == "swept":
            row = {k: int(v) for k, v in (x.split("=") for x in w[1:])}
            out["swept"][row["every"]] = row
        elif w[0] != "==":
            out[w[0]] = [int(x) for x in w[1:]]
    return out


def test_the_story(report):
    """every = 4: a rest of ten frames, a texture update, three more, a cut of two drawn frames, a rest again; then zr_finish."""
    rows = report["story"]
    frames = [r for r in rows if r["kind"] != "ask"]
    asks = [(int(r["frame_no"]), int(r["f"]), int(r["handed"]), int(r["recorded_now"])) for r in rows if r["kind"] == "ask"]
    assert [int(r["frame_no"]) for r in frames] == list(range(18))
    # the first frame of a rest records, then every fourth; a frame that is not one launch, and the first one launch behind it, always do
    assert [int(r["recorded"]) for r in frames] == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0,  0, 0, 1,  1, 1,  1, 1, 0]
    assert asks == [(10, 9, 9, 1),        # the update asks for frame 9's end: nobody recorded it - the stream's tail, now, in frame 9's name
                    (13, 11, 12, 0),      # the cut's head asks for frame 11's: frame 12 recorded its own, a later end serves
                    (14, 12, 12, 0), (15, 13, 13, 0),
                    (18, 17, 17, 1)]      # zr_finish: the newest frame's end, ahead of the wait
    assert report["story_broken"] == [0]


def test_no_sequence_hands_out_a_wrong_end(report):
    s = report["swept"]
    assert sorted(s) == [1, 4, 8]
    for every, row in s.items():
        assert row["sequences"] == 4 * 5 ** 7 + 1 and row["asks"] > row["sequences"] and row["paced"] > 0, row
    assert s[1]["sparse"] == 0 and s[1]["stand_ins"] == 0 and s[1]["recorded_now"] == 0, s[1]      # every frame records: as before the rule
    assert s[8]["sparse"] > s[4]["sparse"] > 0 and s[4]["stand_ins"] > 0 and s[4]["recorded_now"] > 0 and s[8]["recorded_now"] > 0, s
    assert report["broken"] == [0]
