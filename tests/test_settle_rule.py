"""When a resting frame's launch may leave a part's pixels alone, without a GPU (csrc/zr_settle.h: zr_settle_step).

tests/settle_check.cpp is built stand-alone, with the address and undefined-behaviour sanitizers where this machine's g++ links them.
It runs the rule beside a model of one part of the target that knows what the kernel cannot - whether the bytes there are still the
colour they should be - over every sequence of eight frames drawn from: a stand launch like the last, a stand launch with another key,
any other lighting pass, a call that changes the colour behind the kernel's back followed by a stand launch; and again from just below
the wrap of the generation.  What its written-out sequences must print is stated here from the rule ("The
schedule"), not from the program:
  - a pass that is not a stand launch is given generation 0 and ends the standing run;
  - the first stand launch after it, a stand launch with another key and one behind a forget each move on to a generation never used
    before; a stand launch like the one before it keeps its generation;
  - the generation is never 0 on a stand launch, and where it wraps past 2^32 it starts again at 1 behind a wipe of the marks.
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
    d = tmp_path_factory.mktemp("settle_rule")
    hello = d / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    sanitize = SANITIZE if subprocess.call(["g++"] + SANITIZE + [str(hello), "-o", str(d / "hello")], stderr=subprocess.DEVNULL) == 0 and \
        subprocess.call([str(d / "hello")]) == 0 else []
    exe = d / "settle_check"
    subprocess.check_call(["g++"] + FLAGS + sanitize + ["-I", CSRC, os.path.join(ROOT, "tests", "settle_check.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    out, name = {"sequences": {}}, None
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "==":
            name = w[1]
            out["sequences"][name] = []
        elif w[0].startswith("kind="):
            out["sequences"][name].append(dict(x.split("=") for x in w))
        else:
            out[w[0]] = [int(x) if x.isdigit() else x for x in w[1:]]
    return out


def test_the_story(report):
    rows = report["sequences"]["story"]
    assert [r["kind"] for r in rows] == ["other", "other", "stand", "stand", "stand", "stand_new_key", "stand", "other", "stand", "stand", "forget_stand", "stand"]
    assert [int(r["gen"]) for r in rows] == [0, 0, 1, 1, 1, 2, 2, 0, 3, 3, 4, 4]
    assert [int(r["standing"]) for r in rows] == [0, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1]
    assert all(r["wipe"] == "0" for r in rows)
    assert report["story_broken"] == [0]


def test_the_wrap(report):
    rows = report["sequences"]["wrap"]
    assert [int(r["gen"]) for r in rows] == [0xFFFFFFFF, 0xFFFFFFFF, 0, 1, 1, 0, 2]
    assert [int(r["wipe"]) for r in rows] == [0, 0, 0, 1, 0, 0, 0]
    assert report["wrap_broken"] == [0, "wipes", 1]


def test_no_sequence_leaves_a_stale_part_alone(report):
    assert report["swept"][:2] == [4 ** 8, 4 ** 7]
    stands, skips, wipes = report["swept"][3], report["swept"][5], report["swept"][7]
    assert stands > skips > 0 and wipes > 0, report["swept"]      # (parts were left alone, and the wrap was met)
    assert report["broken"] == [0]
