"""Which pass events a timed frame records, and what its figures read, without a GPU (csrc/zr_timed.h: zr_timed_rule).

tests/timed_plan_check.cpp is built stand-alone, with the address and undefined-behaviour sanitizers where this machine's g++ links them.
It drives zr_frame_plan over a scripted run of frames and over every combination of the facts and carry bits that decide which stages a
frame runs, on which stream, and whether it is one launch, and checks the rule's result for each plan.  What it must print is stated here
from the rule ("The schedule"), not from the program:
  - a stage the plan does not run records nothing, and its figures read 0; frame_begin and the lighting's end are always recorded;
  - a frame that keeps its camera pass records one start mark for the lighting's span where it recorded six, and a frame that is one
    launch none: its span starts at frame_begin, on the same stream;
  - a frame that draws its camera pass records exactly what it recorded before the rule, on the same streams.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

DRAWN = "begin,shadow_bins,shadow,cull,round1,hiz,round2,resolve,lighting,camera"      # (in the order of the enum)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("timed_plan")
    hello = d / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    sanitize = SANITIZE if subprocess.call(["g++"] + SANITIZE + [str(hello), "-o", str(d / "hello")], stderr=subprocess.DEVNULL) == 0 and \
        subprocess.call([str(d / "hello")]) == 0 else []
    exe = d / "timed_plan_check"
    subprocess.check_call(["g++"] + FLAGS + sanitize + ["-I", CSRC, os.path.join(ROOT, "tests", "timed_plan_check.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    out, name = {"sequences": {}}, None
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "==":
            name = w[1]
            out["sequences"][name] = []
        elif w[0].startswith("frame="):
            out["sequences"][name].append(dict(x.split("=") for x in w))
        elif w[0] == "seen":
            out["seen"] = {k: int(x) for k, x in (y.split("=") for y in w[1:])}
        else:
            out[w[0]] = [int(x) if x.isdigit() else x for x in w[1:]]
    return out


def test_the_story(report):
    rows = report["sequences"]["story"]
    # drawn, drawn (the map kept: the resolve on the host's stream), the fill, three frames of one launch, a light move, a camera move
    assert [r["camera"] for r in rows] == ["cam", "cam", "none", "none", "none", "none", "none", "cam"]
    assert [r["shadow"] for r in rows] == ["host", "none", "none", "none", "none", "none", "host", "none"]
    assert [int(r["args"]) for r in rows] == [0, 0, 0, 1, 1, 1, 0, 0] and [int(r["fill"]) for r in rows] == [0, 0, 1, 0, 0, 0, 0, 0]
    assert [int(r["n"]) for r in rows] == [10, 12, 3, 2, 2, 2, 5, 12]
    assert rows[0]["set"] == DRAWN and rows[1]["set"] == rows[7]["set"] == DRAWN + ",mark,host_resolve"
    assert rows[2]["set"] == "begin,resolve,lighting" and rows[3]["set"] == rows[4]["set"] == rows[5]["set"] == "begin,lighting"
    assert rows[6]["set"] == "begin,shadow_bins,shadow,resolve,lighting"
    assert [r["lighting_from"] for r in rows] == ["resolve", "resolve", "resolve", "begin", "begin", "begin", "resolve", "resolve"]


def test_every_plan(report):
    assert report["swept"] == [3 * 2 ** 20]
    seen = report["seen"]
    assert all(seen[k] > 0 for k in ("one_launch", "kept_kept", "kept_camera_drawn_map", "drawn_camera", "resolve_deferred", "round2_kept_drawn")), seen
    assert report["broken"] == [0]
