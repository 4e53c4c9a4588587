"""Which kernels a delivery launches, observed from outside the library: tests/frame_delta_launch_probe.py runs once as a child process
under `rocprofv3 --kernel-trace` (a time limit of its own), and the trace's k_delta_* dispatches are read back in the order they started.

A context in mode 1 makes the launches it made before the packed forms existed - k_delta_mark, k_delta_pack per delivery, host form and
device form alike, and nothing of the codec; a packed delivery is k_delta_mark, k_delta_measure, k_delta_encode; a raw delivery of a
context in mode 3 is the raw pair again."""
import csv
import glob
import os
import shutil
import subprocess
import sys

import pytest

import frame_delta_launch_probe as probe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_PAIR = ["k_delta_mark", "k_delta_pack"]
PACKED_TRIPLE = ["k_delta_mark", "k_delta_measure", "k_delta_encode"]


def test_a_mode_1_context_makes_the_launches_it_made_before(gpu_engine, tmp_path):
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(rocprof), "rocprofv3 is what observes the launches"
    out = tmp_path / "trace"
    env = dict(os.environ, TMPDIR=str(tmp_path))
    run = subprocess.run(["timeout", "-k", "10", "120", rocprof, "--kernel-trace", "--output-format", "csv", "-d", str(out), "-o", "probe", "--",
                          sys.executable, os.path.join(ROOT, "tests", "frame_delta_launch_probe.py")],
                         cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=150)
    text = run.stdout.decode(errors="replace")
    assert run.returncode == 0, text[-4000:]
    assert "delivered %d %d %d" % (probe.RAW, probe.PACKED, probe.RAW_BESIDE) in text, text[-4000:]
    traces = glob.glob(str(out / "**" / "*kernel_trace.csv"), recursive=True)
    assert len(traces) == 1, traces
    rows = [r for r in csv.DictReader(open(traces[0])) if "k_delta_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"].replace("void ", "").split("<")[0].split("(")[0] for r in rows]
    assert names == RAW_PAIR * probe.RAW + PACKED_TRIPLE * probe.PACKED + RAW_PAIR * probe.RAW_BESIDE, names
    # a workgroup of 256 threads per tile in every one of them, and the frame's 9 x 5 tiles
    assert {(r["Workgroup_Size_X"], r["Grid_Size_X"]) for r in rows} == {("256", str(256 * 45))}
