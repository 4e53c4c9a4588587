"""Which kernels the staged deliveries launch, and that a wire style which no delivery asks for changes no launch, observed from outside
the library: tests/wire_launch_probe.py runs once as a child process under `rocprofv3 --kernel-trace` (a time limit of its own), and the
trace's k_frame_scale, k_highlight_*, k_delta_* and k_wire_* dispatches are read back in the order they started."""
import csv
import glob
import os
import shutil
import subprocess
import sys

import pytest

import delivery_launch_probe as base
import wire_launch_probe as probe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = ("k_frame_scale", "k_highlight_", "k_delta_", "k_wire_")


def test_a_wire_style_alone_changes_no_launch_and_staged_calls_launch_their_stages(gpu_engine, tmp_path):
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(rocprof), "rocprofv3 is what observes the launches"
    out = tmp_path / "trace"
    env = dict(os.environ, TMPDIR=str(tmp_path))
    run = subprocess.run(["timeout", "-k", "10", "150", rocprof, "--kernel-trace", "--output-format", "csv", "-d", str(out), "-o", "probe", "--",
                          sys.executable, os.path.join(ROOT, "tests", "wire_launch_probe.py")],
                         cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=180)
    text = run.stdout.decode(errors="replace")
    assert run.returncode == 0, text[-4000:]
    assert "delivered %d %d" % (base.FRAMES, base.N_CALLS) in text and "staged %d %d" % (probe.FRAMES, len(probe.CALLS)) in text, text[-4000:]
    traces = glob.glob(str(out / "**" / "*kernel_trace.csv"), recursive=True)
    assert len(traces) == 1, traces
    rows = [r for r in csv.DictReader(open(traces[0])) if any(k in r["Kernel_Name"] for k in OBSERVED)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"].replace("void ", "").split("<")[0].split("(")[0] for r in rows]
    n = len(base.EXPECTED) * base.FRAMES
    assert names[:n] == base.EXPECTED * base.FRAMES, names[:n]           # every existing call: what it launched before
    assert names[n:] == probe.EXPECTED * probe.FRAMES, names[n:]
