"""The lighting pass's keep without a GPU (csrc/zr_frame_plan.h: ZrFramePlan::light_keep / light_fill, ZR_STAGE_LIGHTING).

tests/lighting_keep_plan_check.cpp includes the header alone - plain C++17, nothing of HIP - and is compiled and run here, with the
address and undefined-behaviour sanitizers where this machine's g++ links them for a stand-alone program.  It drives zr_frame_plan and
zr_frame_carry through scripted sequences, one printed line per frame.  What the sequences must print is written out below from the
rule, not from the program: the plane is read by a frame that keeps both its camera pass and its shadow map when it was filled from that
run of GBuffer copies (a), that drawing of the map (b), byte-equal standing uniforms (c), that cubemap (d), in deferred shading (e); a
frame that keeps both but finds no such plane fills it; every other frame ignores it.  A context's first two frames draw (one round, two
rounds); a camera-pass change is followed by two drawn frames, a shadow-pass change by one.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

I, F, R = "ignored", "filled", "read"
REST = [I, I, F, R]                 # drawn, drawn, the first frame that keeps both, the frames after


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    d = tmp_path_factory.mktemp("lighting_keep_plan")
    hello = d / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    sanitize = SANITIZE if subprocess.call(["g++"] + SANITIZE + [str(hello), "-o", str(d / "hello")], stderr=subprocess.DEVNULL) == 0 and \
        subprocess.call([str(d / "hello")]) == 0 else []
    exe = d / "lighting_keep_plan_check"
    subprocess.check_call(["g++"] + FLAGS + sanitize + ["-I", CSRC, os.path.join(ROOT, "tests", "lighting_keep_plan_check.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    out, name = {}, None
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "==":
            name = w[1]
            out[name] = []
        else:
            out[name].append(dict(x.split("=") for x in w))
    return out


def light(report, name):
    rows = report[name]
    assert [r["frame"] for r in rows][:4] == ["0", "1", "2", "3"]
    return [r["light"] for r in rows]


def test_no_plan_both_fills_and_reads_and_every_lighting_pass_is_on_the_hosts_stream(report):
    """One plane is enough because of the second: all lighting passes of a context run in order on one stream."""
    rows = [r for seq in report.values() for r in seq]
    assert len(rows) > 100
    assert all(r["both"] == "0" and r["lighting"] == "host" for r in rows)


@pytest.mark.parametrize("name", ["rest_render", "rest_serial", "rest_staged", "rest_geometry"])
def test_a_rest_fills_once_and_then_reads(report, name):
    """zr_render on two lanes, ZR_FLAG_SERIAL_PASSES, the staged entry points and zr_render_geometry decide alike."""
    assert light(report, name) == REST + [R, R]
    assert [(r["map"], r["pass"]) for r in report[name]] == [("drawn", "drawn"), ("kept", "drawn")] + [("kept", "whole")] * 4


def test_a_fill_or_read_keeps_both_passes(report):
    for name, rows in report.items():
        for r in rows:
            if r["light"] != I:
                assert r["map"] == "kept" and r["pass"] == "whole", (name, r)


def test_no_list_reuse_never_keeps(report):
    assert light(report, "no_list_reuse") == [I] * 6


@pytest.mark.parametrize("name", ["tile_world_2", "shadow_world_2", "stile_world_4"])
def test_partitioned_contexts_never_keep(report, name):
    """Their map is drawn every frame: there is no standing map to keep the shadow factor against."""
    assert light(report, name) == [I] * 6
    assert all(r["map"] == "drawn" for r in report[name])


def test_no_room_for_the_plane_is_no_error_and_never_keeps(report):
    assert light(report, "no_room") == [I] * 6
    assert [r["pass"] for r in report["no_room"]][2:] == ["whole"] * 4         # (the other keeps go on)


@pytest.mark.parametrize("name", ["a_camera_moves", "a_surface_changes"])
def test_a_the_gbuffer_run_ends(report, name):
    """Two frames resolve the two copies again; the third keeps the pass and, the plane being of another run, fills."""
    assert light(report, name) == REST + [I, I, F, R, R]


@pytest.mark.parametrize("name", ["b_light_moves", "b_casters_change"])
def test_b_the_map_is_drawn_again(report, name):
    assert light(report, name) == REST + [I, F, R, R, R]
    assert [r["map"] for r in report[name]][4:6] == ["drawn", "kept"]


def test_b_a_caller_owned_map_is_never_kept(report):
    assert light(report, "b_map_external") == REST + [I, I, I] + [I, F, R, R]


def test_c_the_uniforms_alone(report):
    """GBuffer and map stand: the very next frame fills, and going back to the old values fills again (the plane holds one set)."""
    assert light(report, "c_uniforms_change") == REST + [F, R, R] + [F, R]
    assert all(r["map"] == "kept" and r["pass"] == "whole" for r in report["c_uniforms_change"][2:])


def test_d_the_cubemap_alone(report):
    assert light(report, "d_cubemap_replaced") == REST + [F, R, R]


def test_e_forward_shading_ignores_the_plane(report):
    """(the winner planes come and go with the mode: two frames resolve again each time)"""
    assert light(report, "e_forward_and_back") == REST + [I] * 4 + [I, I, F, R]


def test_the_shortcut_is_part_of_the_key(report):
    """Filled with the shortcut on, the plane lacks the pixels that took it: the first frame without it fills every pixel, and that plane
    serves frames of both kinds."""
    assert light(report, "shortcut_off_and_on") == REST + [F, R] + [R, R] + [R]


def test_a_carry_reset_invalidates_the_plane(report):
    """Every counter starts over and reaches its old values again: the frames repeat the first rest, they do not read."""
    assert light(report, "carry_reset") == REST + REST
    assert light(report, "plane_forgotten") == REST + [F, R]
